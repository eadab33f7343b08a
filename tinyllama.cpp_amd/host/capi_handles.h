// capi_handles.h -- the handles behind include/gten_host.h's opaque types, shared by the host/capi*.cpp files.
#pragma once

#include <memory>

#include "../../include/gten_host.h"
#include "fsm_build.h"
#include "generate.h"
#include "shift_plan.h"
#include "tokenizer.h"

struct gten_host_model {
    gten_host_config cfg;
    std::unique_ptr<gten::TinyLlama> model;
    gten::ShiftCounts shifts;            // include/gten_host_shift.h
};

struct gten_host_batch {
    gten_host_config cfg;
    std::unique_ptr<gten::TinyLlamaBatch> batch;
    gten::ShiftCounts shifts;            // include/gten_host_shift.h
};

struct gten_host_fsm {
    gten::FsmPool pool;
};

struct gten_host_tokenizer {
    Tokenizer tok;
    gten_host_tokenizer(const char* path, int vocab) : tok(path, vocab) {}
};
