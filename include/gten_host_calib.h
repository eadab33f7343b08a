/*
 * gten_host_calib.h -- calibrated Q4 loading: the importance of every block linear's input columns collected from prompt passes,
 * and a linear weight quantised from unquantised elements through the device's delta search; exported by libgten_host.so
 * (host/capi_calib.cpp, host/calib.h).  The device's part is include/gten_hip_calib.h, which defines the search and the column
 * energy; DESIGN.md 3.28.
 *
 * Collection.  Between gten_host_calib_begin and gten_host_calib_end every block forward of a prompt pass of the model
 * (gten_host_model_logits, _score, _score_many, ...: anything that computes rows through the blocks; decoder steps do not
 * collect) adds the rows it computed, from start_pos on, to four per-layer f64 accumulators on the device:
 *     which 0   the input of q | k | v   [n_embd]        which 2   the input of gate | up   [n_embd]
 *     which 1   the input of o           [n_embd]        which 3   the input of down        [n_ffn]
 * One collection at a time per process.
 */
#ifndef GTEN_HOST_CALIB_H
#define GTEN_HOST_CALIB_H

#include "gten_host_quant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* begin: zeroed accumulators, collection on.  end: collection off; the accumulators stay readable until the next begin or the
 * model's end.  0; -1 bad handle, or begin while another model collects / end without begin; else the device library's code. */
int gten_host_calib_begin(gten_host_model* m);
int gten_host_calib_end(gten_host_model* m);

/* rows collected since begin (per layer: every layer sees the same rows); -1 bad handle or never begun */
long long gten_host_calib_rows(gten_host_model* m);

/* the energy of layer `layer`, input `which`: out[c] = sum over the collected rows of element c squared, n its width as above.
 * 0; -1 bad handle, layer, which or pointer, or never begun; -2 n is not the width; else the device library's code. */
int gten_host_calib_read(gten_host_model* m, int layer, int which, double* out, int n);

/* Weight idx (the .gten record order) from its dense elements in src_dtype, as gten_host_model_set_weight_from takes them,
 * quantised through gten_hip_quantize_weight_search with importance f32 [n] (host memory; null with n == cols: every weight 1).
 * Only q, k, v, o, gate, up and down of a block of a Q4 model.
 * 0; -1 bad handle, index, dtype or pointer; -2 wrong size; -3 embed_tokens, lm_head, a norm vector, a model that is not Q4 or
 * n != cols (gten_host_calib_error() names it); else the device library's code with its text in gten_hip_last_error(). */
int gten_host_calib_set_weight_from(gten_host_model* m, int idx, const void* bytes, size_t nbytes, int src_dtype,
                                    const float* importance, int n);

/* the text of the model's last -3 */
const char* gten_host_calib_error(gten_host_model* m);

#ifdef __cplusplus
}
#endif
#endif
