"""ctypes binding of include/gten_host.h (libgten_host.so): the C++ model driver."""
import ctypes as C
import os

import numpy as np

from . import build as _build
from .hipabi import F16, Q8, GtenHipError, load as _load_hip


class HostConfig(C.Structure):
    _fields_ = [(k, C.c_int) for k in
                ("n_vocab", "max_ctx", "n_embd", "n_ffn", "n_layers", "n_heads", "n_kv_heads", "wdtype", "adtype")]

    def weight_shapes(self):
        E, F, V = self.n_embd, self.n_ffn, self.n_vocab
        KV = (E // self.n_heads) * self.n_kv_heads
        W, F16 = self.wdtype, 1
        out = [(V, E, W)]
        for _ in range(self.n_layers):
            out += [(E, E, W), (KV, E, W), (KV, E, W), (E, E, W), (F, E, W), (F, E, W), (E, F, W), (1, E, F16), (1, E, F16)]
        return out + [(1, E, F16), (V, E, W)]


class HostPenalties(C.Structure):
    """gten_host_penalties (include/gten_host_penalty.h)"""
    _fields_ = ([(k, C.c_void_p) for k in ("rep", "freq", "pres", "last_n", "count_prompt")] +
                [(k, C.c_float) for k in ("rep_all", "freq_all", "pres_all")] + [(k, C.c_int32) for k in ("last_n_all", "count_prompt_all")])


def _sig(lib, name, res, args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = args
    return f


class GtenHost:
    SYMBOLS = [
        "gten_host_default_config", "gten_host_model_create", "gten_host_model_free", "gten_host_model_n_weights",
        "gten_host_model_weight_bytes", "gten_host_model_set_weight", "gten_host_model_load_gten",
        "gten_host_model_load_synthetic", "gten_host_model_logits", "gten_host_model_greedy", "gten_host_model_generate",
        "gten_host_tokenizer_create", "gten_host_tokenizer_free", "gten_host_tokenizer_encode", "gten_host_tokenizer_decode",
        "gten_host_synth_weight", "gten_host_write_gten", "gten_host_synthetic_tokens",
        "gten_host_model_set_fast_decode", "gten_host_model_decode_begin", "gten_host_model_decode_step", "gten_host_model_decode_steps", "gten_host_batch_decode_steps",
        "gten_host_model_decode_result", "gten_host_model_time_family",
        "gten_host_batch_create", "gten_host_batch_free", "gten_host_batch_load_synthetic", "gten_host_batch_set_weight",
        "gten_host_batch_prefill", "gten_host_batch_prefill_many", "gten_host_batch_generate", "gten_host_batch_serve", "gten_host_batch_serve2", "gten_host_batch_set_serve_schedule", "gten_host_batch_set_serve_spares", "gten_host_batch_set_serve_ramp", "gten_host_batch_decode_begin", "gten_host_batch_decode_step", "gten_host_batch_decode_step_ragged",
        "gten_host_batch_decode_result", "gten_host_batch_logits", "gten_host_batch_time_family", "gten_host_batch_kv_info", "gten_host_batch_seq_steps",
    ]
    # include/gten_host_sample.h (top-k sampling, host/capi_sample.cpp)
    SAMPLE_SYMBOLS = ["gten_host_model_generate_topk", "gten_host_batch_generate_topk", "gten_host_batch_serve_topk"]
    # include/gten_host_bias.h (bias tables: constrained generation, host/capi_bias.cpp)
    BIAS_SYMBOLS = ["gten_host_model_set_bias_table", "gten_host_batch_set_bias_table", "gten_host_batch_set_sampling", "gten_host_batch_set_seq_bias",
                    "gten_host_batch_bias_info", "gten_host_model_set_seq_bias", "gten_host_model_set_sampling", "gten_host_model_step_logits", "gten_host_model_generate_biased", "gten_host_batch_generate_biased",
                    "gten_host_batch_serve_biased"]
    # include/gten_host_logprobs.h (log-probs and top-N alternatives of the generated ids, host/capi_logprobs.cpp)
    LOGPROBS_SYMBOLS = ["gten_host_model_set_logprobs", "gten_host_batch_set_logprobs", "gten_host_model_logprobs", "gten_host_batch_logprobs",
                        "gten_host_model_generate_lp", "gten_host_batch_generate_lp", "gten_host_batch_serve_lp", "gten_host_model_score_top"]
    LOGPROBS_TOP = 20                                            # GTEN_HIP_LOGPROBS_TOP
    # include/gten_host_nucleus.h (top-p / min-p cuts of the draw, host/capi_nucleus.cpp)
    NUCLEUS_SYMBOLS = ["gten_host_model_set_cut", "gten_host_batch_set_cut", "gten_host_model_cut_info", "gten_host_batch_cut_info",
                       "gten_host_model_generate_nucleus", "gten_host_batch_generate_nucleus", "gten_host_batch_serve_nucleus"]
    # include/gten_host_penalty.h (repetition / frequency / presence penalties, host/capi_penalty.cpp)
    PENALTY_SYMBOLS = ["gten_host_model_set_penalty", "gten_host_batch_set_penalty", "gten_host_model_penalty_info", "gten_host_batch_penalty_info",
                       "gten_host_model_generate_penalized", "gten_host_batch_generate_penalized", "gten_host_batch_serve_penalized"]
    # include/gten_host_fsm.h (token automata: builders, pools and bound generation, host/capi_fsm.cpp)
    FSM_SYMBOLS = ["gten_host_fsm_create", "gten_host_fsm_free", "gten_host_fsm_add_stop", "gten_host_fsm_add_choices", "gten_host_fsm_add_table",
                   "gten_host_fsm_n_states", "gten_host_fsm_tables", "gten_host_model_set_fsm", "gten_host_batch_set_fsm", "gten_host_model_fsm_info",
                   "gten_host_batch_fsm_info", "gten_host_model_set_seq_fsm", "gten_host_batch_set_seq_fsm", "gten_host_model_fsm_states",
                   "gten_host_batch_fsm_states", "gten_host_batch_fsm_decoder", "gten_host_model_generate_fsm", "gten_host_batch_generate_fsm", "gten_host_batch_serve_fsm"]
    # include/gten_host_mirostat.h (a sequence's Mirostat v2 binding on a model's or a batch's decoder)
    MIROSTAT_SYMBOLS = ["gten_host_model_set_mirostat", "gten_host_batch_set_mirostat", "gten_host_model_mirostat_info", "gten_host_batch_mirostat_info",
                        "gten_host_model_mirostat_mus", "gten_host_batch_mirostat_mus", "gten_host_model_generate_mirostat",
                        "gten_host_batch_generate_mirostat", "gten_host_batch_serve_mirostat"]
    # include/gten_host_regex.h (regular expressions as ranges of an automaton pool, host/capi_regex.cpp)
    REGEX_SYMBOLS = ["gten_host_fsm_set_vocab", "gten_host_tokenizer_vocab_bytes", "gten_host_fsm_add_regex", "gten_host_regex_byte_dfa",
                     "gten_host_fsm_n_regex"]
    # include/gten_host_stoptext.h (stop strings given as text) and include/gten_host_json.h (JSON schemas as patterns), host/capi_text.cpp
    STOPTEXT_SYMBOLS = ["gten_host_fsm_add_stop_text", "gten_host_fsm_n_search", "gten_host_stop_text_dfa", "gten_host_stop_text_find"]
    JSON_SYMBOLS = ["gten_host_json_schema_regex"]
    SCORE_SYMBOLS = ["gten_host_model_score", "gten_host_model_logits_all", "gten_host_model_score_many"]   # include/gten_host_score.h
    PREFIX_SYMBOLS = ["gten_host_batch_set_prefix", "gten_host_batch_prefix_info"]                          # include/gten_host_prefix.h
    PREFIX_DECODE_SYMBOLS = ["gten_host_batch_prefix_decode_info", "gten_host_batch_prefix_decode_share",
                             "gten_host_set_prefix_decode_shared"]                                          # include/gten_host_prefix_decode.h
    PREFIXES_SYMBOLS = ["gten_host_batch_prefixes_set", "gten_host_batch_prefixes_info", "gten_host_batch_prefixes_decode_info",
                        "gten_host_batch_prefixes_decode_share", "gten_host_batch_prefixes_steps",
                        "gten_host_prefixes_match"]                                                         # include/gten_host_prefixes.h
    SAMPLES_SYMBOLS = ["gten_host_batch_serve_samples", "gten_host_batch_samples_info", "gten_host_batch_set_groups_cap",
                       "gten_host_batch_group_decode_set", "gten_host_batch_group_decode_share", "gten_host_batch_groups_decode_info",
                       "gten_host_samples_rank", "gten_host_samples_rank_records"]                          # include/gten_host_samples.h
    GROUPS_MAX = 64                                              # GTEN_GROUPS_MAX
    # include/gten_host_sessions.h (continued sequences, host/capi_sessions.cpp)
    SESSIONS_SYMBOLS = ["gten_host_batch_extend_info", "gten_host_batch_extend_many", "gten_host_session_plan", "gten_host_batch_sessions_reserve",
                        "gten_host_batch_session_open", "gten_host_batch_session_close", "gten_host_batch_session_info", "gten_host_batch_session_ids",
                        "gten_host_batch_session_truncate", "gten_host_batch_sessions_info", "gten_host_batch_serve_sessions"]
    SESSIONS_MAX = 256                                           # GTEN_HOST_SESSIONS_MAX
    # include/gten_host_shift.h (context shift: the plan, the cache primitives, generation past the window, host/capi_shift.cpp)
    SHIFT_SYMBOLS = ["gten_host_shift_last_error", "gten_host_shift_plan", "gten_host_shift_drop", "gten_host_shift_phi", "gten_host_model_shift",
                     "gten_host_batch_shift", "gten_host_batch_kv_read", "gten_host_batch_kv_row_bytes", "gten_host_batch_shift_info",
                     "gten_host_model_shift_info", "gten_host_model_generate_shifting", "gten_host_batch_generate_shifting",
                     "gten_host_batch_session_shift"]
    # include/gten_host_embed.h (hidden rows of texts and one pooled vector per text, host/capi_embed.cpp; the plan: host/embed_plan.h)
    EMBED_SYMBOLS = ["gten_host_embed_last_error", "gten_host_embed_plan", "gten_host_model_hidden_many", "gten_host_model_embed_many"]
    POOLINGS = {"mean": 0, "last": 1}                            # GTEN_HOST_POOL_*
    SHIFT_STREAM_MAX = 1 << 24                                   # GTEN_HOST_SHIFT_STREAM_MAX
    # include/gten_host_beam.h (beam search, host/capi_beam.cpp; the plan: host/beam_plan.h)
    BEAM_SYMBOLS = ["gten_host_batch_beam_search", "gten_host_beam_weights", "gten_host_beam_backtrack", "gten_host_beam_finalize"]
    BEAM_MAX = 8                                                 # GTEN_HOST_BEAM_MAX
    # include/gten_host_resident.h (resident weights: what a decoder decided, and the plan: host/resident_plan.h)
    RESIDENT_SYMBOLS = ["gten_host_model_resident", "gten_host_batch_resident", "gten_host_resident_plan"]
    # include/gten_host_ab.h (what a decoder chose among the A/B forms of include/gten_hip_oplanes.h)
    AB_SYMBOLS = ["gten_host_model_o_planes", "gten_host_batch_o_planes"]
    RESIDENT_BLOCK_BYTES = {"f16": 64, "q8": 34, "q4": 18}       # bytes of a 32-element weight block, deltas included
    BEAM_ENDED = ("eos", "length")                               # GTEN_HOST_BEAM_ENDED_*
    SAMPLES_MAX = 64                                             # GTEN_HOST_SAMPLES_MAX

    def __init__(self, path=None):
        path = path or _build.HOST_LIB
        if not os.path.exists(path):
            raise GtenHipError(f"{path} is missing: run __graft_entry__.build()")
        self.hip = _load_hip()                     # libgten_hip.so first (RTLD_GLOBAL)
        self.lib = L = C.CDLL(path)
        vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
        cfgp = C.POINTER(HostConfig)
        self._defcfg = _sig(L, "gten_host_default_config", None, [cfgp, ci, ci])
        self._create = _sig(L, "gten_host_model_create", vp, [cfgp])
        self._free = _sig(L, "gten_host_model_free", None, [vp])
        self._nw = _sig(L, "gten_host_model_n_weights", ci, [vp])
        self._wb = _sig(L, "gten_host_model_weight_bytes", sz, [vp, ci])
        self._setw = _sig(L, "gten_host_model_set_weight", ci, [vp, ci, vp, sz])
        self._loadg = _sig(L, "gten_host_model_load_gten", ci, [vp, C.c_char_p])
        self._loads = _sig(L, "gten_host_model_load_synthetic", ci, [vp, C.c_uint64])
        self._logits = _sig(L, "gten_host_model_logits", ci, [vp, vp, ci, ci, vp])
        self._greedy = _sig(L, "gten_host_model_greedy", ci, [vp, vp, ci, ci, ci])
        self._generate = _sig(L, "gten_host_model_generate", ci, [vp, vp, ci, ci, ci])
        self._generate_topk = _sig(L, "gten_host_model_generate_topk", ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, C.c_uint32])
        self._bserve_topk = _sig(L, "gten_host_batch_serve_topk", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                      C.c_float, C.c_uint64])
        self._bgen_topk = _sig(L, "gten_host_batch_generate_topk", ci, [vp, vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, vp, vp, vp])
        self._m_bias_table = _sig(L, "gten_host_model_set_bias_table", ci, [vp, ci, vp, vp, ci, C.c_float])
        self._b_bias_table = _sig(L, "gten_host_batch_set_bias_table", ci, [vp, ci, vp, vp, ci, C.c_float])
        self._b_set_sampling = _sig(L, "gten_host_batch_set_sampling", ci, [vp, ci, ci, C.c_float, C.c_uint64, C.c_uint32])
        self._b_seq_bias = _sig(L, "gten_host_batch_set_seq_bias", ci, [vp, ci, ci, ci])
        self._m_seq_bias = _sig(L, "gten_host_model_set_seq_bias", ci, [vp, ci, ci])
        self._m_set_sampling = _sig(L, "gten_host_model_set_sampling", ci, [vp, ci, C.c_float, C.c_uint64, C.c_uint32])
        self._m_step_logits = _sig(L, "gten_host_model_step_logits", ci, [vp, vp])
        self._b_bias_info = _sig(L, "gten_host_batch_bias_info", ci, [vp, vp, vp])
        self._generate_biased = _sig(L, "gten_host_model_generate_biased", ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, C.c_uint32, ci, ci])
        self._bgen_biased = _sig(L, "gten_host_batch_generate_biased", ci, [vp, vp, vp, ci, ci, ci, vp, vp, ci, C.c_float, C.c_uint64, vp, vp, vp, vp, vp])
        self._bserve_biased = _sig(L, "gten_host_batch_serve_biased", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                          C.c_float, C.c_uint64, vp, vp])
        self._m_set_lp = _sig(L, "gten_host_model_set_logprobs", ci, [vp, ci])
        self._b_set_lp = _sig(L, "gten_host_batch_set_logprobs", ci, [vp, ci, ci])
        self._m_lp = _sig(L, "gten_host_model_logprobs", ci, [vp, ci, ci, ci, vp, vp, vp])
        self._b_lp = _sig(L, "gten_host_batch_logprobs", ci, [vp, ci, ci, ci, ci, vp, vp, vp])
        self._generate_lp = _sig(L, "gten_host_model_generate_lp", ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, C.c_uint32, ci, ci, ci, vp, vp, vp])
        self._bgen_lp = _sig(L, "gten_host_batch_generate_lp", ci, [vp, vp, vp, ci, ci, ci, vp, vp, ci, C.c_float, C.c_uint64, vp, vp, vp, vp, vp,
                                                                    vp, ci, vp, vp, vp])
        self._bserve_lp = _sig(L, "gten_host_batch_serve_lp", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                  C.c_float, C.c_uint64, vp, vp, vp, ci, vp, vp, vp])
        self._m_set_cut = _sig(L, "gten_host_model_set_cut", ci, [vp, C.c_float, C.c_float])
        self._b_set_cut = _sig(L, "gten_host_batch_set_cut", ci, [vp, ci, C.c_float, C.c_float])
        self._m_cut_info = _sig(L, "gten_host_model_cut_info", ci, [vp, vp, vp, vp])
        self._b_cut_info = _sig(L, "gten_host_batch_cut_info", ci, [vp, vp, vp, vp])
        self._generate_nuc = _sig(L, "gten_host_model_generate_nucleus", ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, C.c_uint32, ci, ci, ci,
                                                                              C.c_float, C.c_float, vp, vp, vp])
        self._bgen_nuc = _sig(L, "gten_host_batch_generate_nucleus", ci, [vp, vp, vp, ci, ci, ci, vp, vp, ci, C.c_float, C.c_uint64, vp, vp, vp, vp, vp,
                                                                          vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float])
        self._bserve_nuc = _sig(L, "gten_host_batch_serve_nucleus", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                         C.c_float, C.c_uint64, vp, vp, vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float])
        pen = C.POINTER(HostPenalties)
        self._m_set_pen = _sig(L, "gten_host_model_set_penalty", ci, [vp, C.c_float, C.c_float, C.c_float, ci, ci])
        self._b_set_pen = _sig(L, "gten_host_batch_set_penalty", ci, [vp, ci, C.c_float, C.c_float, C.c_float, ci, ci])
        self._m_pen_info = _sig(L, "gten_host_model_penalty_info", ci, [vp, vp, vp, vp, vp, vp])
        self._b_pen_info = _sig(L, "gten_host_batch_penalty_info", ci, [vp, vp, vp, vp, vp, vp])
        self._generate_pen = _sig(L, "gten_host_model_generate_penalized", ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, C.c_uint32, ci, ci, ci,
                                                                                C.c_float, C.c_float, vp, vp, vp, pen])
        self._bgen_pen = _sig(L, "gten_host_batch_generate_penalized", ci, [vp, vp, vp, ci, ci, ci, vp, vp, ci, C.c_float, C.c_uint64, vp, vp, vp, vp, vp,
                                                                            vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float, pen])
        self._bserve_pen = _sig(L, "gten_host_batch_serve_penalized", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                           C.c_float, C.c_uint64, vp, vp, vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float, pen])
        self._fsm_create = _sig(L, "gten_host_fsm_create", vp, [ci])
        self._fsm_free = _sig(L, "gten_host_fsm_free", None, [vp])
        self._fsm_add_stop = _sig(L, "gten_host_fsm_add_stop", ci, [vp, vp, vp, ci])
        self._fsm_add_choices = _sig(L, "gten_host_fsm_add_choices", ci, [vp, vp, vp, ci])
        self._fsm_add_table = _sig(L, "gten_host_fsm_add_table", ci, [vp, vp, vp, ci])
        self._fsm_n_states = _sig(L, "gten_host_fsm_n_states", ci, [vp])
        self._fsm_tables = _sig(L, "gten_host_fsm_tables", ci, [vp, C.POINTER(vp), C.POINTER(vp)])
        self._fsm_set_vocab = _sig(L, "gten_host_fsm_set_vocab", ci, [vp, vp, vp])
        self._tok_vocab_bytes = _sig(L, "gten_host_tokenizer_vocab_bytes", C.c_longlong, [vp, ci, vp, ci, vp, C.c_longlong, vp])
        self._fsm_add_regex = _sig(L, "gten_host_fsm_add_regex", ci, [vp, C.c_char_p, ci, C.POINTER(ci)])
        self._regex_byte_dfa = _sig(L, "gten_host_regex_byte_dfa", ci, [C.c_char_p, vp, vp, ci, C.POINTER(ci)])
        self._fsm_n_regex = _sig(L, "gten_host_fsm_n_regex", ci, [vp])
        self._fsm_add_stop_text = _sig(L, "gten_host_fsm_add_stop_text", ci, [vp, vp, vp, ci])
        self._fsm_n_search = _sig(L, "gten_host_fsm_n_search", ci, [vp])
        self._stop_text_dfa = _sig(L, "gten_host_stop_text_dfa", ci, [vp, vp, ci, vp, vp, ci])
        self._stop_text_find = _sig(L, "gten_host_stop_text_find", ci, [vp, vp, ci, vp, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)])
        self._json_schema_regex = _sig(L, "gten_host_json_schema_regex", C.c_longlong, [C.c_char_p, ci, ci, vp, C.c_longlong, vp, C.c_longlong])
        self._m_set_fsm = _sig(L, "gten_host_model_set_fsm", ci, [vp, vp])
        self._b_set_fsm = _sig(L, "gten_host_batch_set_fsm", ci, [vp, vp])
        self._m_set_mirostat = _sig(L, "gten_host_model_set_mirostat", ci, [vp, C.c_float, C.c_float, C.c_int32, ci])
        self._b_set_mirostat = _sig(L, "gten_host_batch_set_mirostat", ci, [vp, ci, C.c_float, C.c_float, C.c_int32, ci])
        self._m_mirostat_info = _sig(L, "gten_host_model_mirostat_info", ci, [vp, vp, vp, vp])
        self._b_mirostat_info = _sig(L, "gten_host_batch_mirostat_info", ci, [vp, vp, vp, vp])
        self._m_mirostat_mus = _sig(L, "gten_host_model_mirostat_mus", ci, [vp, ci, ci, vp])
        self._b_mirostat_mus = _sig(L, "gten_host_batch_mirostat_mus", ci, [vp, ci, ci, ci, vp])
        self._m_fsm_info = _sig(L, "gten_host_model_fsm_info", ci, [vp, C.POINTER(ci), vp, vp])
        self._b_fsm_info = _sig(L, "gten_host_batch_fsm_info", ci, [vp, C.POINTER(ci), vp, vp])
        self._m_set_seq_fsm = _sig(L, "gten_host_model_set_seq_fsm", ci, [vp, ci, ci])
        self._b_set_seq_fsm = _sig(L, "gten_host_batch_set_seq_fsm", ci, [vp, ci, ci, ci])
        self._m_fsm_states = _sig(L, "gten_host_model_fsm_states", ci, [vp, ci, ci, vp])
        self._b_fsm_states = _sig(L, "gten_host_batch_fsm_states", ci, [vp, ci, ci, ci, vp])
        self._b_fsm_decoder = _sig(L, "gten_host_batch_fsm_decoder", vp, [vp])
        ll, llp = C.c_longlong, C.POINTER(C.c_longlong)
        self._m_resident = _sig(L, "gten_host_model_resident", ci, [vp, C.POINTER(ci), llp, llp, llp])
        self._b_resident = _sig(L, "gten_host_batch_resident", ci, [vp, C.POINTER(ci), llp, llp, llp])
        self._m_o_planes = _sig(L, "gten_host_model_o_planes", ci, [vp, C.POINTER(ci)])
        self._b_o_planes = _sig(L, "gten_host_batch_o_planes", ci, [vp, C.POINTER(ci)])
        self._resident_plan = _sig(L, "gten_host_resident_plan", ci, [ci, ci, ci, ci, ci, ci, ll, vp, vp, llp])
        self._generate_fsm = _sig(L, "gten_host_model_generate_fsm", ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, C.c_uint32, ci, ci, ci,
                                                                          C.c_float, C.c_float, vp, vp, vp, pen, ci, vp])
        self._bgen_fsm = _sig(L, "gten_host_batch_generate_fsm", ci, [vp, vp, vp, ci, ci, ci, vp, vp, ci, C.c_float, C.c_uint64, vp, vp, vp, vp, vp,
                                                                      vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float, pen, vp, vp])
        self._bserve_fsm = _sig(L, "gten_host_batch_serve_fsm", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                     C.c_float, C.c_uint64, vp, vp, vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float, pen,
                                                                     vp, vp])
        self._generate_miro = _sig(L, "gten_host_model_generate_mirostat", ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, C.c_uint32, ci, ci, ci,
                                                                                C.c_float, C.c_float, vp, vp, vp, pen, ci, vp, C.c_float, C.c_float])
        self._bgen_miro = _sig(L, "gten_host_batch_generate_mirostat", ci, [vp, vp, vp, ci, ci, ci, vp, vp, ci, C.c_float, C.c_uint64, vp, vp, vp, vp, vp,
                                                                            vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float, pen, vp, vp,
                                                                            vp, vp, C.c_float, C.c_float])
        self._bserve_miro = _sig(L, "gten_host_batch_serve_mirostat", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                           C.c_float, C.c_uint64, vp, vp, vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float, pen,
                                                                           vp, vp, vp, vp, C.c_float, C.c_float])
        self._bserve_sessions = _sig(L, "gten_host_batch_serve_sessions", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                               C.c_float, C.c_uint64, vp, vp, vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float, pen,
                                                                               vp, vp, vp])
        self._bsess_reserve = _sig(L, "gten_host_batch_sessions_reserve", ci, [vp, ci])
        self._bsess_open = _sig(L, "gten_host_batch_session_open", ci, [vp])
        self._bsess_close = _sig(L, "gten_host_batch_session_close", ci, [vp, ci])
        self._bsess_info = _sig(L, "gten_host_batch_session_info", ci, [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)])
        self._bsess_ids = _sig(L, "gten_host_batch_session_ids", ci, [vp, ci, vp, ci])
        self._bsess_truncate = _sig(L, "gten_host_batch_session_truncate", ci, [vp, ci, ci])
        _ull = C.c_ulonglong
        self._bsessions_info = _sig(L, "gten_host_batch_sessions_info", ci, [vp, C.POINTER(ci), C.POINTER(_ull), C.POINTER(_ull), C.POINTER(_ull),
                                                                             C.POINTER(_ull), C.POINTER(_ull)])
        self._score_top = _sig(L, "gten_host_model_score_top", ci, [vp, vp, ci, ci, vp, ci, vp, vp, vp, vp])
        self._score = _sig(L, "gten_host_model_score", ci, [vp, vp, ci, ci, vp, vp, vp])
        self._logits_all = _sig(L, "gten_host_model_logits_all", ci, [vp, vp, ci, ci, vp])
        self._score_many = _sig(L, "gten_host_model_score_many", ci, [vp, vp, vp, ci, vp, vp, vp])
        self._tok_create = _sig(L, "gten_host_tokenizer_create", vp, [C.c_char_p, ci])
        self._tok_free = _sig(L, "gten_host_tokenizer_free", None, [vp])
        self._tok_encode = _sig(L, "gten_host_tokenizer_encode", ci, [vp, C.c_char_p, ci, vp, ci])
        self._tok_decode = _sig(L, "gten_host_tokenizer_decode", C.c_char_p, [vp, ci, ci])
        self._setfast = _sig(L, "gten_host_model_set_fast_decode", ci, [vp, ci])
        self._dbegin = _sig(L, "gten_host_model_decode_begin", ci, [vp, vp, ci])
        self._dstep = _sig(L, "gten_host_model_decode_step", ci, [vp, ci, ci])
        self._dsteps = _sig(L, "gten_host_model_decode_steps", ci, [vp, ci, ci, ci])
        self._bsteps = _sig(L, "gten_host_batch_decode_steps", ci, [vp, ci, ci, ci])
        self._dresult = _sig(L, "gten_host_model_decode_result", ci, [vp, ci, C.POINTER(C.c_int32)])
        self._timefam = _sig(L, "gten_host_model_time_family", ci, [vp, ci, ci, ci, C.POINTER(C.c_double), C.POINTER(ci)])
        self._bcreate = _sig(L, "gten_host_batch_create", vp, [cfgp, ci])
        self._bfree = _sig(L, "gten_host_batch_free", None, [vp])
        self._bloads = _sig(L, "gten_host_batch_load_synthetic", ci, [vp, C.c_uint64])
        self._bsetw = _sig(L, "gten_host_batch_set_weight", ci, [vp, ci, vp, sz])
        self._bprefill = _sig(L, "gten_host_batch_prefill", ci, [vp, ci, vp, ci, vp])
        self._bprefill_many = _sig(L, "gten_host_batch_prefill_many", ci, [vp, vp, vp, vp, ci, vp])
        self._bbegin = _sig(L, "gten_host_batch_decode_begin", ci, [vp, ci, vp, ci])
        self._bstep = _sig(L, "gten_host_batch_decode_step", ci, [vp, ci, ci])
        self._bstepr = _sig(L, "gten_host_batch_decode_step_ragged", ci, [vp, vp, ci])
        self._bgen = _sig(L, "gten_host_batch_generate", ci, [vp, vp, vp, ci, ci, ci, vp, vp])
        self._bserve = _sig(L, "gten_host_batch_serve2", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci])
        self._bsched = _sig(L, "gten_host_batch_set_serve_schedule", ci, [vp, ci])
        self._bspares = _sig(L, "gten_host_batch_set_serve_spares", ci, [vp, ci])
        self._bramp = _sig(L, "gten_host_batch_set_serve_ramp", ci, [vp, ci])
        self._bresult = _sig(L, "gten_host_batch_decode_result", ci, [vp, ci, ci, C.POINTER(C.c_int32)])
        self._blogits = _sig(L, "gten_host_batch_logits", ci, [vp, ci, vp])
        self._btime = _sig(L, "gten_host_batch_time_family", ci, [vp, ci, ci, ci, C.POINTER(C.c_double), C.POINTER(ci)])
        self._bseqsteps = _sig(L, "gten_host_batch_seq_steps", ci, [vp, ci, vp, ci, ci, ci])
        self._bkvinfo = _sig(L, "gten_host_batch_kv_info", ci, [vp, C.POINTER(ci), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])
        self._bsetprefix = _sig(L, "gten_host_batch_set_prefix", ci, [vp, vp, ci])
        self._bprefixinfo = _sig(L, "gten_host_batch_prefix_info", ci, [vp, C.POINTER(ci), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])
        self._bpdinfo = _sig(L, "gten_host_batch_prefix_decode_info", ci,
                             [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])
        self._bpdshare = _sig(L, "gten_host_batch_prefix_decode_share", ci, [vp, ci, ci])
        self._pdshared = _sig(L, "gten_host_set_prefix_decode_shared", ci, [ci])
        ull = C.c_ulonglong
        self._bpsset = _sig(L, "gten_host_batch_prefixes_set", ci, [vp, ci, vp, ci])
        self._bpsinfo = _sig(L, "gten_host_batch_prefixes_info", ci, [vp, ci, C.POINTER(ci), C.POINTER(ull), C.POINTER(ull)])
        self._bpsdinfo = _sig(L, "gten_host_batch_prefixes_decode_info", ci,
                              [vp, ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(ci), C.POINTER(ull), C.POINTER(ci)])
        self._bpsdshare = _sig(L, "gten_host_batch_prefixes_decode_share", ci, [vp, ci, ci, ci])
        self._bpssteps = _sig(L, "gten_host_batch_prefixes_steps", ci, [vp, ci, vp, ci, ci, ci])
        self._psmatch = _sig(L, "gten_host_prefixes_match", ci, [vp, vp, ci, ci, vp, ci])
        self._bserve_samples = _sig(L, "gten_host_batch_serve_samples", ci, [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, ci, vp, vp, ci,
                                                                             C.c_float, C.c_uint64, vp, vp, vp, ci, vp, vp, vp, vp, vp, C.c_float, C.c_float, pen,
                                                                             vp, vp, vp, ci])
        self._bsamples_info = _sig(L, "gten_host_batch_samples_info", ci, [vp, C.POINTER(ull), C.POINTER(ull), C.POINTER(ull), C.POINTER(ull), C.POINTER(ci)])
        self._bgroups_cap = _sig(L, "gten_host_batch_set_groups_cap", ci, [vp, ci])
        self._bextend_many = _sig(L, "gten_host_batch_extend_many", ci, [vp, vp, vp, vp, vp, ci, vp, vp])
        self._bextend_info = _sig(L, "gten_host_batch_extend_info", ci, [vp, C.POINTER(ull), C.POINTER(ull), C.POINTER(ull), C.POINTER(ull)])
        self._session_plan = _sig(L, "gten_host_session_plan", ci, [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)])
        self._bbeam = _sig(L, "gten_host_batch_beam_search", ci, [vp, vp, vp, ci, ci, ci, ci, C.c_float, vp, vp, vp, vp, vp, vp, C.POINTER(ci)])
        self._beam_weights = _sig(L, "gten_host_beam_weights", ci, [ci, C.c_float, vp])
        self._beam_backtrack = _sig(L, "gten_host_beam_backtrack", ci, [vp, vp, ci, ci, ci, vp])
        self._beam_finalize = _sig(L, "gten_host_beam_finalize", ci, [vp, vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, vp])
        self._bgdset = _sig(L, "gten_host_batch_group_decode_set", ci, [vp, ci, ci, ci])
        self._bgdshare = _sig(L, "gten_host_batch_group_decode_share", ci, [vp, ci, ci, ci])
        self._bgdinfo = _sig(L, "gten_host_batch_groups_decode_info", ci, [vp, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ull), C.POINTER(ci)])
        self._samples_rank = _sig(L, "gten_host_samples_rank", ci, [vp, vp, ci, vp])
        self._samples_rank_records = _sig(L, "gten_host_samples_rank_records", ci, [vp, ci, ci, vp, ci, vp])
        self._synthw = _sig(L, "gten_host_synth_weight", ci, [cfgp, C.c_uint64, ci, vp, sz])
        self._writeg = _sig(L, "gten_host_write_gten", ci, [cfgp, C.c_uint64, C.c_char_p])
        self._stoks = _sig(L, "gten_host_synthetic_tokens", None, [vp, ci, C.c_uint32, ci])
        self._shift_err = _sig(L, "gten_host_shift_last_error", C.c_char_p, [])
        self._shift_plan = _sig(L, "gten_host_shift_plan", ci, [ci, ci, ci, ci, ci] + [C.POINTER(ci)] * 5)
        self._shift_drop = _sig(L, "gten_host_shift_drop", ci, [ci, ci, ci])
        self._shift_phi = _sig(L, "gten_host_shift_phi", ci, [ci, ci, ci])
        self._mshift = _sig(L, "gten_host_model_shift", ci, [vp, ci, ci, ci])
        self._bshift = _sig(L, "gten_host_batch_shift", ci, [vp, vp, vp, ci, ci, ci])
        self._bkv_read = _sig(L, "gten_host_batch_kv_read", ci, [vp, ci, ci, ci, ci, vp, vp])
        self._bkv_row_bytes = _sig(L, "gten_host_batch_kv_row_bytes", ci, [vp])
        self._bshift_info = _sig(L, "gten_host_batch_shift_info", ci, [vp, C.POINTER(ull), C.POINTER(ull), C.POINTER(ull)])
        self._mshift_info = _sig(L, "gten_host_model_shift_info", ci, [vp, C.POINTER(ull), C.POINTER(ull), C.POINTER(ull)])
        self._generate_shift = _sig(L, "gten_host_model_generate_shifting", ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, C.c_uint32, ci, ci, C.c_float,
                                                                                C.c_float, pen, ci, ci])
        self._bgen_shift = _sig(L, "gten_host_batch_generate_shifting", ci, [vp, vp, vp, ci, ci, ci, ci, C.c_float, C.c_uint64, vp, ci, ci, C.c_float, C.c_float,
                                                                             pen, ci, ci, vp, vp])
        self._bsess_shift = _sig(L, "gten_host_batch_session_shift", ci, [vp, ci, ci, ci])
        self._embed_err = _sig(L, "gten_host_embed_last_error", C.c_char_p, [])
        self._embed_plan = _sig(L, "gten_host_embed_plan", ci, [vp, ci, ci, vp, vp])
        self._hidden_many = _sig(L, "gten_host_model_hidden_many", ci, [vp, vp, vp, ci, ci, vp, C.POINTER(ci)])
        self._embed_many = _sig(L, "gten_host_model_embed_many", ci, [vp, vp, vp, ci, ci, ci, ci, vp])

    def shift_error(self):
        """the text of the last refusal by an entry point of include/gten_host_shift.h"""
        return self._shift_err().decode(errors="replace")

    # -- the context shift's plan (host/shift_plan.h): no device needed
    def shift_plan(self, n_ids, rows, max_ctx, keep, drop=0):
        """(due, keep, drop, ids after, rows after) for a sequence of n_ids ids, `rows` of them with valid K / V rows; None: no such plan"""
        o = [C.c_int(0) for _ in range(5)]
        if self._shift_plan(int(n_ids), int(rows), int(max_ctx), int(keep), int(drop), *[C.byref(x) for x in o]):
            return None
        return tuple(x.value for x in o)

    def shift_drop(self, rows, keep, drop=0):
        """the drop that applies to `rows` valid rows, or -1 where shift(keep, drop) is not possible on them"""
        return self._shift_drop(int(rows), int(keep), int(drop))

    def shift_phi(self, p, keep, drop):
        return self._shift_phi(int(p), int(keep), int(drop))

    def embed_error(self):
        """the text of the last refusal by an entry point of include/gten_host_embed.h"""
        return self._embed_err().decode(errors="replace")

    # -- the embedding calls' plan (host/embed_plan.h): no device needed
    def embed_plan(self, lengths, seg_ok=True):
        """(group of every text, [1 where the group is a text that goes alone]) for texts of these lengths; None: no such plan"""
        a = np.ascontiguousarray(lengths, dtype=np.int32)
        group_of, alone = np.zeros(max(len(a), 1), np.int32), np.zeros(max(len(a), 1), np.int32)
        n = self._embed_plan(a.ctypes.data_as(C.c_void_p), len(a), 1 if seg_ok else 0, group_of.ctypes.data_as(C.c_void_p), alone.ctypes.data_as(C.c_void_p))
        if n < 0:
            return None
        return [int(g) for g in group_of[: len(a)]], [int(x) for x in alone[:n]]

    def default_config(self, wdtype, adtype):
        cfg = HostConfig()
        self._defcfg(C.byref(cfg), wdtype, adtype)
        return cfg

    def synth_weight(self, cfg, seed, idx):
        rows, cols, dt = cfg.weight_shapes()[idx]
        out = np.zeros(rows * self.hip.row_bytes(dt, cols), np.uint8)
        rc = self._synthw(C.byref(cfg), seed, idx, out.ctypes.data_as(C.c_void_p), out.size)
        if rc:
            raise GtenHipError(f"gten_host_synth_weight rc={rc}")
        return out

    def write_gten(self, cfg, seed, path):
        rc = self._writeg(C.byref(cfg), seed, path.encode())
        if rc:
            raise GtenHipError(f"gten_host_write_gten rc={rc}")

    def set_prefix_decode_shared(self, on):
        """process-wide: decode slots behind a shared prefix read one copy of its K / V (default) or each its own"""
        rc = self._pdshared(-1 if on is None else 1 if on else 0)    # (None: the default again)
        if rc:
            raise GtenHipError(f"gten_host_set_prefix_decode_shared rc={rc}")

    def samples_rank(self, logprob_sum, n_new):
        """gten_host_samples_rank (include/gten_host_samples.h; no device): the samples' indices, best first -- descending mean
        log-prob per new id (logprob_sum[i] / n_new[i] in double), ties to the lower sample, samples without new ids last"""
        sums, nn = np.ascontiguousarray(logprob_sum, dtype=np.float64), np.ascontiguousarray(n_new, dtype=np.int32)
        assert len(sums) == len(nn)
        order = np.zeros(max(len(nn), 1), np.int32)
        rc = self._samples_rank(_ptr(sums), _ptr(nn), len(nn), _ptr(order))
        if rc:
            raise ValueError(f"samples_rank rc={rc}")
        return order[: len(nn)].copy()

    def samples_rank_records(self, records, n_prompt, n_new):
        """... with the sums formed from the samples' f32 log-prob rows (records [n][width]; new ids from position n_prompt on)"""
        rec, nn = np.ascontiguousarray(records, dtype=np.float32), np.ascontiguousarray(n_new, dtype=np.int32)
        assert rec.ndim == 2 and rec.shape[0] == len(nn)
        order = np.zeros(max(len(nn), 1), np.int32)
        rc = self._samples_rank_records(_ptr(rec), rec.shape[1], int(n_prompt), _ptr(nn), len(nn), _ptr(order))
        if rc:
            raise ValueError(f"samples_rank_records rc={rc}")
        return order[: len(nn)].copy()

    def prefixes_match(self, prefixes, prompt):
        """gten_host_prefixes_match (include/gten_host_prefixes.h): the index of the longest of `prefixes` (id lists; empty or None: not
        registered) that `prompt` begins with and has at least 16 ids behind, the lower index among equal lengths; -1: none"""
        prefixes = [[] if p is None else list(p) for p in prefixes]
        lens = np.ascontiguousarray([len(p) for p in prefixes], dtype=np.int32)
        max_len = int(lens.max()) if len(prefixes) else 0
        flat = np.zeros((max(len(prefixes), 1), max(max_len, 1)), np.int32)
        for i, p in enumerate(prefixes):
            flat[i, :len(p)] = p
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        return self._psmatch(flat.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), len(prefixes), max(max_len, 1),
                             prompt.ctypes.data_as(C.c_void_p), len(prompt))

    # -- beam search's plan (host/beam_plan.h): no device needed
    def beam_weights(self, max_new, length_penalty):
        """f32[max_new + 1]: w[0] = 0, w[t] = (float)(1 / t^length_penalty)"""
        w = np.zeros(max_new + 1, np.float32)
        if self._beam_weights(int(max_new), float(length_penalty), _ptr(w)):
            raise GtenHipError("beam_weights: bad arguments")
        return w

    def beam_backtrack(self, parent, ids, t, b):
        """the ids of beam b after round t; parent / ids int32[rows][8], round r at row r - 1.  None where the walk leaves the trellis"""
        parent, ids = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1, 8), np.ascontiguousarray(ids, dtype=np.int32).reshape(-1, 8)
        out = np.zeros(max(int(t), 1), np.int32)
        n = self._beam_backtrack(_ptr(parent), _ptr(ids), len(parent), int(t), int(b), _ptr(out))
        return None if n < 0 else out[:n].copy()

    def beam_finalize(self, state, parent, ids, n_beams, w, max_new):
        """state: one 176-byte record (hipabi.GtenHip.BEAM_STATE); returns [(ids, final, cum, ended_by)], best first"""
        parent, ids = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1, 8), np.ascontiguousarray(ids, dtype=np.int32).reshape(-1, 8)
        st = np.frombuffer(np.asarray(state).tobytes(), np.uint8).copy()
        assert st.size == 176
        w = np.ascontiguousarray(w, dtype=np.float32)
        oi, on = np.zeros((n_beams, max_new), np.int32), np.zeros(n_beams, np.int32)
        of, oc, oe = np.zeros(n_beams, np.float32), np.zeros(n_beams, np.float32), np.zeros(n_beams, np.int32)
        n = self._beam_finalize(_ptr(st), _ptr(parent), _ptr(ids), len(parent), int(n_beams), _ptr(w), int(max_new), _ptr(oi), _ptr(on), _ptr(of), _ptr(oc), _ptr(oe))
        if n < 0:
            raise GtenHipError("beam_finalize: bad arguments")
        return [(oi[i, : on[i]].copy(), of[i], oc[i], self.BEAM_ENDED[oe[i]]) for i in range(n)]

    def session_plan(self, n_ids, rows, n_new, segmented=True):
        """gten_host_session_plan (include/gten_host_sessions.h): (rows kept, rows computed, path 0 whole / 1 continued / 2 one by
        one) of a turn of n_new ids behind n_ids ids with `rows` valid K / V rows; None where there is no such turn"""
        ctx, k, path = C.c_int(0), C.c_int(0), C.c_int(0)
        if self._session_plan(int(n_ids), int(rows), int(n_new), 1 if segmented else 0, C.byref(ctx), C.byref(k), C.byref(path)) != 0:
            return None
        return ctx.value, k.value, path.value

    def synthetic_tokens(self, count, seed=12345, n_vocab=32003):
        out = np.zeros(count, np.int32)
        self._stoks(out.ctypes.data_as(C.c_void_p), count, seed, n_vocab)
        return out

    def resident_plan(self, n_layers, n_embd, n_ffn, kv_width, n_vocab, block_bytes, budget):
        """host/resident_plan.h on the W.x launches of one step (per layer q|k|v, o, gate|up, down; then lm_head) against `budget`
        bytes: (resident u8[4 * n_layers + 1], every launch's weight bytes i64[...], resident launches, their byte sum)"""
        n = 4 * n_layers + 1
        res, each, total = np.zeros(n, np.uint8), np.zeros(n, np.int64), C.c_longlong(0)
        got = self._resident_plan(n_layers, n_embd, n_ffn, kv_width, n_vocab, block_bytes, int(budget), _ptr(res), _ptr(each), C.byref(total))
        if got < 0:
            raise GtenHipError(f"resident_plan rc={got}")
        return res, each, got, total.value

    def _resident_of(self, fn, h):
        n, b, budget, over = C.c_int(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        rc = fn(h, C.byref(n), C.byref(b), C.byref(budget), C.byref(over))
        if rc:
            raise GtenHipError(f"resident rc={rc}: {self.hip._err().decode(errors='replace')}")
        return n.value, b.value, budget.value, over.value

    def _o_planes_of(self, fn, h):
        p = C.c_int(-1)
        rc = fn(h, C.byref(p))
        if rc:
            raise GtenHipError(f"o_planes rc={rc}: {self.hip._err().decode(errors='replace')}")
        return p.value

    def model(self, cfg):
        return HostModel(self, cfg)

    def batch(self, cfg, n_seq):
        return HostBatch(self, cfg, n_seq)

    def tokenizer(self, path, vocab_size=32000):
        """host/tokenizer.h on a vocabulary file (host only: no GPU needed)"""
        return HostTokenizer(self, path, vocab_size)

    # ---- stop strings as text and JSON schemas (include/gten_host_stoptext.h, include/gten_host_json.h): device-free
    def stop_text_dfa(self, strings):
        """the strings' Aho-Corasick automaton over bytes (host/stop_text_build.h): (next256 u16 [Sb][256], total; accept u8 [Sb]); a
        refusal raises ValueError with the code"""
        return stop_text_dfa(self, strings)

    def stop_text_find(self, strings, text):
        """(index, begin, end) of the match that ends first in `text` (then the longest, then the lowest index); (-1, n, n) for none"""
        return stop_text_find(self, strings, text)

    def json_schema_regex(self, schema, ws=0, depth=2):
        """the schema (a dict, or its JSON text) as a pattern of the regex dialect; a refusal raises JsonSchemaError"""
        return json_schema_regex(self, schema, ws, depth)


def bias_pairs(pairs=(), fill=0.0, allow=None):
    """(ids int32[], values f32[], fill) of a bias table request (include/gten_hip_bias.h): `pairs` = [(id, value)] over `fill` for every
    other id; allow=[ids] is the shorthand for "only these ids": fill -inf, the ids at 0 (pairs may still bias or ban some of them)."""
    if allow is not None:
        merged = {int(i): 0.0 for i in allow}
        if len(merged) != len(list(allow)):
            raise ValueError("allow lists an id twice")
        for i, v in pairs:
            if int(i) in merged:
                merged[int(i)] = float(v)
            else:
                raise ValueError(f"pair id {i} is not among the allowed ids")
        pairs, fill = list(merged.items()), -np.inf
    ids = np.ascontiguousarray([int(i) for i, _ in pairs], dtype=np.int32)
    values = np.ascontiguousarray([float(v) for _, v in pairs], dtype=np.float32)
    return ids, values, float(fill)


SERVE_STATS = ("prompt_tokens", "new_tokens", "steps", "admissions", "prefill_s", "decode_s", "lane_steps", "lane_rows", "moved")


def _ptr(a):
    """a numpy array (or None) as a C pointer argument; the pointer keeps the array alive"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pack(prompts):
    """(prompts as one zero-padded int32 matrix [n][longest], lengths int32 [n], longest)"""
    mp = max(len(p) for p in prompts)
    pr, npr = np.zeros((len(prompts), mp), np.int32), np.zeros(len(prompts), np.int32)
    for j, p in enumerate(prompts):
        pr[j, : len(p)] = p
        npr[j] = len(p)
    return pr, npr, mp


def _each(v, n, dt, full=False):
    """(array or None, scalar) of a per-item list or one value for all; full: the one value becomes an array too (None stays None)"""
    if v is None:
        return None, None
    if np.isscalar(v):
        return (np.full(n, v, dt), None) if full else (None, v)
    a = np.ascontiguousarray(v, dtype=dt)
    assert len(a) == n
    return a, None


def _request_args(n, top_k, temp, seed):
    """top_k / temp (a scalar or one value per item) and the seed as the C ABI takes them: arrays or null, then the values for all"""
    (ks, k1), (ts, t1) = _each(top_k, n, np.int32), _each(temp, n, np.float32)
    return [_ptr(ks), _ptr(ts), 0 if ks is not None else int(k1), 1.0 if ts is not None else float(t1), C.c_uint64(int(seed))]


def _full_args(n, *pairs):
    """(value, dtype) pairs -- streams, tables, min_new: None, one value for all or one per item -- as full arrays or null"""
    return [_ptr(_each(v, n, dt, full=True)[0]) for v, dt in pairs]


def _n_tops(n_top, n):
    """(int32[n] or None, width of the outputs) of a per-item n_top request (a scalar: for all; None / -1: that item does not ask)"""
    if n_top is None:
        return None, 0
    a = np.full(n, n_top, np.int32) if np.isscalar(n_top) else np.ascontiguousarray([-1 if v is None else v for v in n_top], dtype=np.int32)
    assert len(a) == n
    return a, max(int(a.max()), 0)


def _records(n_top, n, width):
    """the record arguments behind a per-item n_top request, and the outputs they fill: ([n_top, widest, lp, ids, lps], (lp, ids, lps))"""
    nt, tw = _n_tops(n_top, n)
    lp, ti, tl = np.zeros((n, width), np.float32), np.full((n, width, tw), -1, np.int32), np.zeros((n, width, tw), np.float32)
    return [_ptr(nt), tw, _ptr(lp), _ptr(ti), _ptr(tl)], (lp, ti, tl)


def _samples_counts(n, n_prompts):
    """int32[n_prompts] samples per prompt of a scalar for all or one value per prompt"""
    ns = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (n_prompts,)))
    assert ns.min() >= 1 and ns.max() <= GtenHost.SAMPLES_MAX, "samples per prompt in [1, 64]"
    return ns


def _cut_args(n, top_p, min_p):
    """top_p / min_p (a scalar or one value per item) as the C ABI takes them: arrays or null, then the values for all"""
    (ps, p1), (ms, m1) = _each(top_p, n, np.float32), _each(min_p, n, np.float32)
    return [_ptr(ps), _ptr(ms), C.c_float(1.0 if ps is not None else float(p1)), C.c_float(0.0 if ms is not None else float(m1))]


def _penalty_arg(n, rep, freq, pres, last_n, count_prompt):
    """the gten_host_penalties of a call: each value a scalar for everybody or one per item.  The struct keeps its arrays alive."""
    (r, r1), (f, f1), (p, p1) = _each(rep, n, np.float32), _each(freq, n, np.float32), _each(pres, n, np.float32)
    (l, l1), (c, c1) = _each(last_n, n, np.int32), _each([int(bool(v)) for v in count_prompt] if not np.isscalar(count_prompt) else int(bool(count_prompt)), n, np.int32)
    s = HostPenalties(_ptr(r), _ptr(f), _ptr(p), _ptr(l), _ptr(c), 1.0 if r is not None else float(r1), 0.0 if f is not None else float(f1),
                      0.0 if p is not None else float(p1), 0 if l is not None else int(l1), 1 if c is not None else int(c1))
    s._keep = (r, f, p, l, c)
    return s


class RegexError(ValueError):
    def __init__(self, code, offset, pattern):
        super().__init__(f"regex {pattern!r} refused: {code} at byte {offset}")
        self.code, self.offset = code, offset


def vocab_arrays(pieces):
    """a list of bytes objects as (bytes u8[], offsets int32[n + 1])"""
    off = np.zeros(len(pieces) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in pieces])
    return np.frombuffer(b"".join(bytes(p) for p in pieces), np.uint8).copy(), off


def byte_dfa(host, pattern):
    """the pattern's canonical minimal byte automaton (host/regex_build.h): (next256 u16 [Sb][256] with 0xFFFF for no edge, accept u8 [Sb]);
    a refusal raises RegexError"""
    data = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
    off = C.c_int(-1)
    n = host._regex_byte_dfa(data, None, None, 0, C.byref(off))
    if n < 0:
        raise RegexError(n, off.value, pattern)
    n256, acc = np.zeros((n, 256), np.uint16), np.zeros(n, np.uint8)
    host._regex_byte_dfa(data, _ptr(n256), _ptr(acc), n, C.byref(off))
    return n256, acc


def _as_bytes(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def _byte_strings(strings):
    """a list of str / bytes as the C interface's (pointers, lengths): (ptrs, lens, n); the tuple keeps the buffers alive"""
    data = [np.frombuffer(_as_bytes(s) + b"\0", np.uint8).copy() for s in strings]          # (never empty: the pointer is real)
    ptrs = (C.c_void_p * max(len(data), 1))(*[d.ctypes.data for d in data])
    lens = np.ascontiguousarray([len(d) - 1 for d in data], dtype=np.int32)
    ptrs._keep = data
    return ptrs, lens, len(data)


def stop_text_dfa(host, strings):
    ptrs, lens, n = _byte_strings(strings)
    S = host._stop_text_dfa(ptrs, _ptr(lens), n, None, None, 0)
    if S < 0:
        raise ValueError(f"stop_text_dfa refused: {S}")
    n256, acc = np.zeros((S, 256), np.uint16), np.zeros(S, np.uint8)
    host._stop_text_dfa(ptrs, _ptr(lens), n, _ptr(n256), _ptr(acc), S)
    return n256, acc


def stop_text_find(host, strings, text):
    ptrs, lens, n = _byte_strings(strings)
    raw = _as_bytes(text)
    buf = np.frombuffer(raw + b"\0", np.uint8).copy()
    b, e = C.c_longlong(0), C.c_longlong(0)
    k = host._stop_text_find(ptrs, _ptr(lens), n, _ptr(buf), len(raw), C.byref(b), C.byref(e))
    if k < -1:
        raise ValueError(f"stop_text_find refused: {k}")
    return k, int(b.value), int(e.value)


def _cut_text(host, vocab, new_ids, strings):
    """the bytes the new ids spell over `vocab` (Fsm.vocab), cut before the first stop string (stop_text_find)"""
    vb, vo = vocab
    raw = b"".join(bytes(vb[vo[i]:vo[i + 1]]) for i in new_ids)
    return raw[:stop_text_find(host, strings, raw)[1]] if strings else raw


class JsonSchemaError(ValueError):
    """.code -1: malformed JSON, .where the byte offset (int, or None); .code -4: outside the subset, .where the offending key's path"""

    def __init__(self, code, where):
        super().__init__(f"JSON schema refused: {code} at {where!r}")
        self.code, self.where = code, where


def json_schema_regex(host, schema, ws=0, depth=2):
    import json
    text = schema if isinstance(schema, (str, bytes)) else json.dumps(schema, ensure_ascii=False)
    data = _as_bytes(text)
    if b"\0" in data:
        raise JsonSchemaError(-1, data.index(b"\0"))
    err = C.create_string_buffer(1024)
    n = host._json_schema_regex(data, int(ws), int(depth), None, 0, err, len(err))
    if n < 0:
        where = err.value.decode("utf-8", errors="replace")
        raise JsonSchemaError(int(n), (int(where) if where else None) if n == -1 else where)
    out = C.create_string_buffer(n + 1)
    host._json_schema_regex(data, int(ws), int(depth), out, n + 1, err, len(err))
    return out.value.decode("utf-8")


class Fsm:
    """An automaton pool under construction (include/gten_host_fsm.h, host/fsm_build.h): no device needed.  add_stop / add_choices /
    add_table append an automaton and return its start state; a refusal raises ValueError with the builder's code and leaves the
    pool as it was."""

    def __init__(self, host, n_vocab):
        self.host, self.n_vocab = host, int(n_vocab)
        self.h = host._fsm_create(self.n_vocab)
        if not self.h:
            raise ValueError(f"Fsm: n_vocab {n_vocab} outside [1, 65535]")

    @staticmethod
    def _lists(seqs):
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in seqs])
        ids = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32).reshape(-1) for s in seqs]) if len(seqs) else [], dtype=np.int32)
        return ids, off

    def _add(self, fn, what, seqs):
        ids, off = self._lists(seqs)
        rc = fn(self.h, _ptr(ids) if len(ids) else None, _ptr(off), len(seqs))
        if rc < 0:
            raise ValueError(f"{what} refused: {rc}")
        return rc

    def add_stop(self, seqs):
        """Aho-Corasick over the id sequences: nothing banned, final wherever one of them ends; the start state"""
        return self._add(self.host._fsm_add_stop, "add_stop", seqs)

    def add_choices(self, seqs):
        """a trie: only its edges allowed, a choice's last id enters a final state; the start state"""
        return self._add(self.host._fsm_add_choices, "add_choices", seqs)

    def add_table(self, nxt, flags):
        """the caller's own automaton (u16 [S][n_vocab], u8 [S]) relocated into the pool; the start state (its state 0)"""
        nxt, flags = np.ascontiguousarray(nxt, dtype=np.uint16), np.ascontiguousarray(flags, dtype=np.uint8)
        assert nxt.shape == (len(flags), self.n_vocab)
        rc = self.host._fsm_add_table(self.h, _ptr(nxt), _ptr(flags), len(flags))
        if rc < 0:
            raise ValueError(f"add_table refused: {rc}")
        return rc

    # ---- regular expressions (include/gten_host_regex.h)
    def set_vocab(self, vocab):
        """the pool's vocabulary as byte strings: a HostTokenizer (its vocab_bytes(n_vocab)), a list of n_vocab bytes objects, or a
        (bytes u8[], offsets int32[n_vocab + 1]) pair.  Needed before add_regex."""
        if isinstance(vocab, HostTokenizer):
            vocab = vocab.vocab_bytes(self.n_vocab)
        elif not (isinstance(vocab, tuple) and len(vocab) == 2):
            vocab = vocab_arrays(vocab)
        vb, vo = np.ascontiguousarray(vocab[0], dtype=np.uint8), np.ascontiguousarray(vocab[1], dtype=np.int32)
        if len(vo) != self.n_vocab + 1:
            raise ValueError(f"set_vocab: {len(vo) - 1} pieces for {self.n_vocab} ids")
        rc = self.host._fsm_set_vocab(self.h, _ptr(vb) if len(vb) else None, _ptr(vo))
        if rc < 0:
            raise ValueError(f"set_vocab refused: {rc}")
        self.vocab = (vb, vo)

    def add_regex(self, pattern, eos=-1):
        """the pattern (str) as a range of the pool: its start state.  A refusal raises RegexError (a ValueError) with .code (-1 syntax,
        -2 too many states, -4 an unsupported construct) and .offset, the byte offset of the offence."""
        off = C.c_int(-1)
        rc = self.host._fsm_add_regex(self.h, pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern), int(eos), C.byref(off))
        if rc < 0:
            raise RegexError(rc, off.value, pattern)
        return rc

    @property
    def n_regex(self):
        return self.host._fsm_n_regex(self.h)

    def byte_dfa(self, pattern):
        return byte_dfa(self.host, pattern)

    # ---- stop strings as text, JSON schemas (include/gten_host_stoptext.h, include/gten_host_json.h)
    def add_stop_text(self, strings):
        """the strings (str as UTF-8, or bytes) as a SEARCH range of the pool: nothing is banned, the id whose bytes complete one of them
        enters the range's HIT state, which is final; the start state.  Needs set_vocab.  A refusal raises ValueError with the code."""
        ptrs, lens, n = _byte_strings(strings)
        rc = self.host._fsm_add_stop_text(self.h, ptrs, _ptr(lens), n)
        if rc < 0:
            raise ValueError(f"add_stop_text refused: {rc}")
        return rc

    @property
    def n_search(self):
        return self.host._fsm_n_search(self.h)

    def add_json_schema(self, schema, eos, ws=0, depth=2):
        """add_regex of json_schema_regex(schema, ws, depth): the start state.  Refusals: JsonSchemaError from the schema, RegexError (-2:
        too many states) from the pattern."""
        return self.add_regex(json_schema_regex(self.host, schema, ws, depth), eos)

    @property
    def n_states(self):
        return self.host._fsm_n_states(self.h)

    def tables(self):
        """copies of the pool: (next u16 [S][n_vocab], flags u8 [S])"""
        n, f = C.c_void_p(), C.c_void_p()
        S = self.host._fsm_tables(self.h, C.byref(n), C.byref(f))
        if S <= 0:
            return np.zeros((0, self.n_vocab), np.uint16), np.zeros(0, np.uint8)
        nxt = np.ctypeslib.as_array(C.cast(n, C.POINTER(C.c_uint16)), shape=(S, self.n_vocab)).copy()
        flags = np.ctypeslib.as_array(C.cast(f, C.POINTER(C.c_uint8)), shape=(S,)).copy()
        return nxt, flags

    def close(self):
        if self.h:
            self.host._fsm_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


MIRO_MU_DEFAULT = -(1 << 31)                                    # GTEN_HIP_MIRO_MU_DEFAULT: mu starts at 2 * tau_q


def _mirostat_info(fn, h, n):
    tq, eq, ps = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    on = fn(h, _ptr(tq), _ptr(eq), _ptr(ps))
    if on < 0:
        raise GtenHipError(f"mirostat_info rc={on}")
    return tq, eq, ps, bool(on)


def _fsm_info(fn, h, n):
    st, ps, S = np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_int(0)
    on = fn(h, C.byref(S), _ptr(st), _ptr(ps))
    if on < 0:
        raise GtenHipError(f"fsm_info rc={on}")
    return S.value, st, ps, bool(on)


class HostTokenizer:
    def __init__(self, host, path, vocab_size):
        self.host = host
        self.h = host._tok_create(str(path).encode(), vocab_size)
        if not self.h:
            raise GtenHipError(f"tokenizer: cannot open {path}")

    def encode(self, prompt, chat_template=True):
        data = prompt if isinstance(prompt, bytes) else prompt.encode("utf-8")
        cap = 16 + 2 * len(data)
        buf = np.zeros(cap, np.int32)
        n = self.host._tok_encode(self.h, data, 1 if chat_template else 0, buf.ctypes.data_as(C.c_void_p), cap)
        if n < 0:
            raise GtenHipError(f"tokenizer_encode rc={n}")
        return buf[:n].tolist()

    def decode(self, prev_token, token):
        return self.host._tok_decode(self.h, prev_token, token)        # bytes

    def vocab_bytes(self, n_vocab, empty=None):
        """the byte strings of ids [0, n_vocab) as decode prints them ("<0xHH>" as the byte, no dropped space): (bytes u8[], offsets
        int32[n_vocab + 1]); ids past the tokenizer and the ids of `empty` (None: 0, 1, 2) are empty (include/gten_host_regex.h)"""
        off = np.zeros(n_vocab + 1, np.int32)
        e = np.ascontiguousarray(empty, dtype=np.int32) if empty is not None else None
        args = (self.h, int(n_vocab), _ptr(e) if e is not None and len(e) else None, len(e) if e is not None else 0)
        if e is not None and len(e) == 0:                                # "nothing is empty": an id outside the vocabulary
            e = np.array([-1], np.int32)
            args = (self.h, int(n_vocab), _ptr(e), 1)
        n = self.host._tok_vocab_bytes(*args, None, 0, _ptr(off))
        if n < 0:
            raise GtenHipError(f"tokenizer_vocab_bytes rc={n}")
        buf = np.zeros(max(n, 1), np.uint8)
        self.host._tok_vocab_bytes(*args, _ptr(buf), n, _ptr(off))
        return buf[:n], off

    def close(self):
        if self.h:
            self.host._tok_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostModel:
    """The C++ TinyLlama driver on the GPU (needs an initialised device)."""

    def __init__(self, host, cfg):
        self.host = host
        self.cfg = cfg
        if host.hip.device_count() < 1:
            raise GtenHipError("no MI355X visible: the model runs only on the gten_hip path")
        self.h = host._create(C.byref(cfg))

    def n_weights(self):
        return self.host._nw(self.h)

    def weight_bytes(self, idx):
        return self.host._wb(self.h, idx)

    def set_weight(self, idx, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        rc = self.host._setw(self.h, idx, data.ctypes.data_as(C.c_void_p), data.size)
        if rc:
            raise GtenHipError(f"set_weight({idx}) rc={rc}")

    def load_gten(self, path):
        rc = self.host._loadg(self.h, path.encode())
        if rc:
            raise GtenHipError(f"load_gten({path}) rc={rc}")

    def load_synthetic(self, seed):
        rc = self.host._loads(self.h, seed)
        if rc:
            raise GtenHipError(f"load_synthetic rc={rc}")

    def logits(self, tokens, start_pos, want=True):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.zeros(self.cfg.n_vocab, np.float32) if want else None
        rc = self.host._logits(self.h, tokens.ctypes.data_as(C.c_void_p), len(tokens), start_pos,
                               out.ctypes.data_as(C.c_void_p) if want else None)
        if rc:
            raise GtenHipError(f"logits rc={rc}")
        return out

    def score_rc(self, tokens, start_pos=0, targets=None):
        """(return code, log-probs f32[n - start_pos], ranks int32[n - start_pos]) of gten_host_model_score (include/gten_host_score.h).
        Row start_pos + i is scored against targets[i]; by default the next id, tokens[start_pos + 1:] + [-1] (-1: not scored)."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        rows = max(len(tokens) - start_pos, 1)
        if targets is None:
            targets = np.append(tokens[start_pos + 1:], -1)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        if len(targets) < rows:
            targets = np.append(targets, np.full(rows - len(targets), -1, np.int32))
        lp, rk = np.zeros(rows, np.float32), np.zeros(rows, np.int32)
        rc = self.host._score(self.h, tokens.ctypes.data_as(C.c_void_p), len(tokens), start_pos, targets.ctypes.data_as(C.c_void_p),
                              lp.ctypes.data_as(C.c_void_p), rk.ctypes.data_as(C.c_void_p))
        return rc, lp, rk

    def score(self, tokens, start_pos=0, targets=None, n_top=None):
        """(log-probs, ranks) of rows [start_pos, n): see score_rc.  With n_top (0 .. 20) also the top-N of every scored row:
        (log-probs, ranks, top ids int32[rows][n_top], top log-probs f32[rows][n_top]) (gten_host_model_score_top)"""
        if n_top is not None:
            return self.score_top(tokens, start_pos, targets, n_top)
        rc, lp, rk = self.score_rc(tokens, start_pos, targets)
        if rc:
            raise GtenHipError(f"score rc={rc}")
        return lp, rk

    def score_top(self, tokens, start_pos=0, targets=None, n_top=0):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        rows = max(len(tokens) - start_pos, 1)
        if targets is None:
            targets = np.append(tokens[start_pos + 1:], -1)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        if len(targets) < rows:
            targets = np.append(targets, np.full(rows - len(targets), -1, np.int32))
        lp, rk = np.zeros(rows, np.float32), np.zeros(rows, np.int32)
        ti, tl = np.full((rows, max(int(n_top), 0)), -1, np.int32), np.zeros((rows, max(int(n_top), 0)), np.float32)
        rc = self.host._score_top(self.h, tokens.ctypes.data_as(C.c_void_p), len(tokens), start_pos, targets.ctypes.data_as(C.c_void_p), int(n_top),
                                  lp.ctypes.data_as(C.c_void_p), rk.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p),
                                  tl.ctypes.data_as(C.c_void_p))
        if rc:
            raise GtenHipError(f"score_top rc={rc}")
        return lp, rk, ti, tl

    def logits_all(self, tokens, start_pos=0):
        """f32 [n - start_pos][n_vocab]: the lm_head of every computed row (gten_host_model_logits_all)"""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.zeros((len(tokens) - start_pos, self.cfg.n_vocab), np.float32)
        rc = self.host._logits_all(self.h, tokens.ctypes.data_as(C.c_void_p), len(tokens), start_pos, out.ctypes.data_as(C.c_void_p))
        if rc:
            raise GtenHipError(f"logits_all rc={rc}")
        return out

    def score_many_rc(self, texts, targets=None):
        """(return code, [log-probs per text], [ranks per text]) of gten_host_model_score_many: every text scored from position 0
        against its next ids (by default) or targets[k]"""
        texts = [np.ascontiguousarray(t, dtype=np.int32) for t in texts]
        if targets is None:
            targets = [np.append(t[1:], -1) for t in texts]
        starts = np.zeros(len(texts) + 1, np.int32)
        starts[1:] = np.cumsum([len(t) for t in texts])
        toks = np.ascontiguousarray(np.concatenate(texts) if texts else np.zeros(0, np.int32), dtype=np.int32)
        tg = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32) for t in targets]) if texts else np.zeros(0, np.int32), dtype=np.int32)
        total = int(starts[-1])
        lp, rk = np.zeros(max(total, 1), np.float32), np.zeros(max(total, 1), np.int32)
        rc = self.host._score_many(self.h, toks.ctypes.data_as(C.c_void_p), starts.ctypes.data_as(C.c_void_p), len(texts),
                                   tg.ctypes.data_as(C.c_void_p), lp.ctypes.data_as(C.c_void_p), rk.ctypes.data_as(C.c_void_p))
        return rc, [lp[starts[k]:starts[k + 1]].copy() for k in range(len(texts))], [rk[starts[k]:starts[k + 1]].copy() for k in range(len(texts))]

    def score_many(self, texts, targets=None):
        """([log-probs per text], [ranks per text]): see score_many_rc"""
        rc, lp, rk = self.score_many_rc(texts, targets)
        if rc:
            raise GtenHipError(f"score_many rc={rc}")
        return lp, rk

    @staticmethod
    def _texts(texts):
        texts = [np.ascontiguousarray(t, dtype=np.int32).reshape(-1) for t in texts]
        starts = np.zeros(len(texts) + 1, np.int32)
        starts[1:] = np.cumsum([len(t) for t in texts])
        toks = np.ascontiguousarray(np.concatenate(texts) if texts else np.zeros(0, np.int32), dtype=np.int32)
        return (toks if len(toks) else np.zeros(1, np.int32)), starts

    def hidden_many_rc(self, texts, layer=None):
        """(return code, [(row bytes uint8[len][row bytes], dtype code) per text]) of gten_host_model_hidden_many (include/gten_host_embed.h):
        every text's rows behind the final norm, in storage form.  layer None: the model's own output."""
        toks, starts = self._texts(texts)
        rb = max(self.host.hip.row_bytes(Q8, self.cfg.n_embd), self.host.hip.row_bytes(F16, self.cfg.n_embd))
        rows = np.zeros((max(int(starts[-1]), 1), rb), np.uint8)
        dt = C.c_int(-1)
        rc = self.host._hidden_many(self.h, toks.ctypes.data_as(C.c_void_p), starts.ctypes.data_as(C.c_void_p), len(texts), 0 if layer is None else int(layer),
                                    rows.ctypes.data_as(C.c_void_p), C.byref(dt))
        if rc:
            return rc, []
        rb = self.host.hip.row_bytes(dt.value, self.cfg.n_embd)
        flat = rows.reshape(-1)[: int(starts[-1]) * rb].reshape(-1, rb)
        return 0, [(flat[starts[k]:starts[k + 1]].copy(), dt.value) for k in range(len(texts))]

    def hidden_many(self, texts, layer=None):
        """[(row bytes, dtype code) per text]: see hidden_many_rc; rows_to_f32 gives the values"""
        rc, rows = self.hidden_many_rc(texts, layer)
        if rc:
            raise GtenHipError(f"hidden_many rc={rc}: {self.host.embed_error()}")
        return rows

    @staticmethod
    def rows_to_f32(rows, dtype):
        """the f32 values of rows in storage form (uint8 [n][row bytes]): Q8 (float)q * f16_to_f32(delta), one f32 multiply; f16 the conversion"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        if dtype == F16:
            return rows.view(np.float16).astype(np.float32)
        assert dtype == Q8
        blk = rows.reshape(rows.shape[0], -1, 34)
        d = np.ascontiguousarray(blk[:, :, :2]).view(np.float16).astype(np.float32)
        q = np.ascontiguousarray(blk[:, :, 2:]).view(np.int8).astype(np.float32)
        return (q * d).astype(np.float32).reshape(rows.shape[0], -1)

    def embed_many_rc(self, texts, pooling="mean", normalize=True, layer=None):
        """(return code, f32 [len(texts)][n_embd]) of gten_host_model_embed_many: one vector per text, pooled (and normalised) on the device"""
        toks, starts = self._texts(texts)
        out = np.zeros((max(len(texts), 1), self.cfg.n_embd), np.float32)
        code = self.host.POOLINGS.get(pooling, pooling)
        rc = self.host._embed_many(self.h, toks.ctypes.data_as(C.c_void_p), starts.ctypes.data_as(C.c_void_p), len(texts), int(code), 1 if normalize else 0,
                                   0 if layer is None else int(layer), out.ctypes.data_as(C.c_void_p))
        return rc, out[: len(texts)]

    def embed_many(self, texts, pooling="mean", normalize=True, layer=None):
        """f32 [len(texts)][n_embd]: see embed_many_rc"""
        rc, out = self.embed_many_rc(texts, pooling, normalize, layer)
        if rc:
            raise GtenHipError(f"embed_many rc={rc}: {self.host.embed_error()}")
        return out

    def embed(self, ids, pooling="mean", normalize=True, layer=None):
        """the vector of one text: embed_many([ids])[0]"""
        return self.embed_many([ids], pooling, normalize, layer)[0]

    def set_fast_decode(self, on):
        self.host._setfast(self.h, 1 if on else 0)

    def decode_begin(self, tokens):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        rc = self.host._dbegin(self.h, tokens.ctypes.data_as(C.c_void_p), len(tokens))
        if rc:
            raise GtenHipError(f"decode_begin rc={rc}")

    def decode_step(self, n, use_graph=True):
        rc = self.host._dstep(self.h, n, 1 if use_graph else 0)
        if rc:
            raise GtenHipError(f"decode_step({n}) rc={rc}")

    def decode_steps(self, n_first, count, use_graph=True):
        """asynchronous: steps n_first .. n_first + count - 1 (ids from decode_begin), four steps per graph replay"""
        rc = self.host._dsteps(self.h, n_first, count, 1 if use_graph else 0)
        if rc:
            raise GtenHipError(f"decode_steps({n_first}, {count}) rc={rc}")

    def decode_result(self, n):
        out = C.c_int32(-1)
        rc = self.host._dresult(self.h, n, C.byref(out))
        if rc:
            raise GtenHipError(f"decode_result({n}) rc={rc}")
        return out.value

    def time_family(self, family, n, reps=20):
        """(average us per launch, launches per replay) of one kernel family, HIP-event timed"""
        us, cnt = C.c_double(0.0), C.c_int(0)
        rc = self.host._timefam(self.h, family, n, reps, C.byref(us), C.byref(cnt))
        if rc:
            raise GtenHipError(f"time_family rc={rc}")
        return us.value, cnt.value

    def greedy(self, prompt, max_tokens, eos=-1):
        buf = np.zeros(max_tokens, np.int32)
        buf[: len(prompt)] = prompt
        total = self.host._greedy(self.h, buf.ctypes.data_as(C.c_void_p), len(prompt), max_tokens, eos)
        return buf[:total].copy()

    def generate(self, prompt, max_tokens, eos=-1):
        """greedy ids with the sampler on the device (gten_host_model_generate): same ids as greedy()"""
        buf = np.zeros(max_tokens, np.int32)
        buf[: len(prompt)] = prompt
        total = self.host._generate(self.h, buf.ctypes.data_as(C.c_void_p), len(prompt), max_tokens, eos)
        return buf[:total].copy()

    def generate_topk(self, prompt, max_tokens, eos, top_k, temp, seed, stream=0):
        """generate() with every new id drawn by the device sampler (include/gten_host_sample.h; top_k 0: greedy)"""
        buf = np.zeros(max(max_tokens, len(prompt)), np.int32)
        buf[: len(prompt)] = prompt
        total = self.host._generate_topk(self.h, buf.ctypes.data_as(C.c_void_p), len(prompt), max_tokens, eos, int(top_k), float(temp),
                                         C.c_uint64(int(seed)), C.c_uint32(int(stream)))
        if total < 0:
            raise GtenHipError(f"generate_topk rc={total}")
        return buf[:total].copy()

    def set_bias_table_rc(self, table, pairs=(), fill=0.0, allow=None):
        """gten_host_model_set_bias_table's return code (0, or the refusal: the table keeps its contents)"""
        ids, values, fill = bias_pairs(pairs, fill, allow)
        return self.host._m_bias_table(self.h, int(table), ids.ctypes.data_as(C.c_void_p), values.ctypes.data_as(C.c_void_p), len(ids), C.c_float(fill))

    def set_bias_table(self, table, pairs=(), fill=0.0, allow=None):
        """bias table `table` of this model's decoder := fill everywhere, then value at id for (id, value) in pairs; allow=[ids]:
        only these ids (include/gten_host_bias.h)"""
        rc = self.set_bias_table_rc(table, pairs, fill, allow)
        if rc:
            raise GtenHipError(f"set_bias_table rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def set_seq_bias_rc(self, table, until=0):
        return self.host._m_seq_bias(self.h, int(table), int(until))

    def set_sampling(self, top_k, temp=1.0, seed=0, stream=0):
        """the request of the steps the caller drives (decode_step): top_k 0 = greedy"""
        rc = self.host._m_set_sampling(self.h, int(top_k), float(temp), C.c_uint64(int(seed)), C.c_uint32(int(stream)))
        if rc:
            raise GtenHipError(f"set_sampling rc={rc}")

    def step_logits(self):
        """the logits row of the last decode step (f32 [n_vocab])"""
        out = np.zeros(self.cfg.n_vocab, np.float32)
        rc = self.host._m_step_logits(self.h, out.ctypes.data_as(C.c_void_p))
        if rc:
            raise GtenHipError(f"step_logits rc={rc}")
        return out

    def generate_biased(self, prompt, max_tokens, eos=-1, top_k=0, temp=1.0, seed=0, stream=0, table=-1, min_new=0):
        """generate_topk() under bias table `table` (-1: none), which holds for the first min_new new ids (0: all); top_k 0: greedy"""
        buf = np.zeros(max(max_tokens, len(prompt)), np.int32)
        buf[: len(prompt)] = prompt
        total = self.host._generate_biased(self.h, buf.ctypes.data_as(C.c_void_p), len(prompt), max_tokens, eos, int(top_k), float(temp),
                                           C.c_uint64(int(seed)), C.c_uint32(int(stream)), int(table), int(min_new))
        if total < 0:
            raise GtenHipError(f"generate_biased rc={total}")
        return buf[:total].copy()

    def set_logprobs_rc(self, n_top):
        return self.host._m_set_lp(self.h, int(n_top))

    def set_logprobs(self, n_top):
        """the decoder's steps commit a log-prob record with n_top alternatives from now on (-1: off; include/gten_host_logprobs.h)"""
        rc = self.set_logprobs_rc(n_top)
        if rc:
            raise GtenHipError(f"set_logprobs rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def logprobs(self, n_from, count, n_top):
        """(logprob f32[count], top_id int32[count][n_top], top_logprob f32[count][n_top]) of positions [n_from, n_from + count)"""
        lp, ti, tl = np.zeros(count, np.float32), np.full((count, n_top), -1, np.int32), np.zeros((count, n_top), np.float32)
        rc = self.host._m_lp(self.h, int(n_from), int(count), int(n_top), lp.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p),
                             tl.ctypes.data_as(C.c_void_p))
        if rc:
            raise GtenHipError(f"logprobs rc={rc}: {self.host.hip._err().decode(errors='replace')}")
        return lp, ti, tl

    def generate_logprobs(self, prompt, max_tokens, n_top, eos=-1, top_k=0, temp=1.0, seed=0, stream=0, table=-1, min_new=0):
        """generate_biased() plus every new id's record: (ids, logprob f32[len(ids)], top_id int32[len(ids)][n_top], top_logprob);
        prompt positions hold 0 / -1"""
        width = max(max_tokens, len(prompt))
        buf = np.zeros(width, np.int32)
        buf[: len(prompt)] = prompt
        lp, ti, tl = np.zeros(width, np.float32), np.full((width, n_top), -1, np.int32), np.zeros((width, n_top), np.float32)
        total = self.host._generate_lp(self.h, buf.ctypes.data_as(C.c_void_p), len(prompt), max_tokens, eos, int(top_k), float(temp),
                                       C.c_uint64(int(seed)), C.c_uint32(int(stream)), int(table), int(min_new), int(n_top),
                                       lp.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p), tl.ctypes.data_as(C.c_void_p))
        if total < 0:
            raise GtenHipError(f"generate_logprobs rc={total}: {self.host.hip._err().decode(errors='replace')}")
        return buf[:total].copy(), lp[:total].copy(), ti[:total].copy(), tl[:total].copy()

    def set_cut_rc(self, top_p, min_p):
        return self.host._m_set_cut(self.h, C.c_float(top_p), C.c_float(min_p))

    def set_cut(self, top_p=1.0, min_p=0.0):
        """the decoder's sampled steps draw under the cut (top_p, min_p) from now on ((1, 0): off; include/gten_host_nucleus.h)"""
        rc = self.set_cut_rc(top_p, min_p)
        if rc:
            raise GtenHipError(f"set_cut rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def resident(self):
        """(resident W.x launches, their weight bytes, the bytes the decoder had left for them, what it took off the setting first)
        of this model's decoder (include/gten_host_resident.h)"""
        return self.host._resident_of(self.host._m_resident, self.h)

    def o_planes(self):
        """1 where this model's decoder runs its o launch as four K-quarter planes, else 0 (include/gten_host_resident.h)"""
        return self.host._o_planes_of(self.host._m_o_planes, self.h)

    def cut_info(self):
        """(top_p, min_p, t = f32(log(min_p)), whether the decoder has ever had a cut set)"""
        a, b, t = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
        on = self.host._m_cut_info(self.h, _ptr(a), _ptr(b), _ptr(t))
        if on < 0:
            raise GtenHipError(f"cut_info rc={on}")
        return a[0], b[0], t[0], bool(on)

    def generate_nucleus(self, prompt, max_tokens, eos=-1, top_k=0, temp=1.0, seed=0, stream=0, top_p=1.0, min_p=0.0, table=-1, min_new=0,
                         n_top=None):
        """generate_biased() with the draw cut by (top_p, min_p) (include/gten_host_nucleus.h); n_top None: the ids; otherwise
        generate_logprobs()'s tuple (ids, logprob, top_id, top_logprob)"""
        width = max(max_tokens, len(prompt))
        buf = np.zeros(width, np.int32)
        buf[: len(prompt)] = prompt
        ask = n_top is not None and n_top >= 0
        w = int(n_top) if ask else 0
        lp, ti, tl = np.zeros(width, np.float32), np.full((width, w), -1, np.int32), np.zeros((width, w), np.float32)
        total = self.host._generate_nuc(self.h, _ptr(buf), len(prompt), max_tokens, eos, int(top_k), float(temp), C.c_uint64(int(seed)),
                                        C.c_uint32(int(stream)), int(table), int(min_new), w if ask else -1, C.c_float(top_p), C.c_float(min_p),
                                        _ptr(lp) if ask else None, _ptr(ti) if ask else None, _ptr(tl) if ask else None)
        if total < 0:
            raise GtenHipError(f"generate_nucleus rc={total}: {self.host.hip._err().decode(errors='replace')}")
        ids = buf[:total].copy()
        return (ids, lp[:total].copy(), ti[:total].copy(), tl[:total].copy()) if ask else ids

    def set_penalty_rc(self, rep, freq=0.0, pres=0.0, start=0, last_n=0):
        return self.host._m_set_pen(self.h, C.c_float(rep), C.c_float(freq), C.c_float(pres), int(start), int(last_n))

    def set_penalty(self, rep=1.0, freq=0.0, pres=0.0, start=0, last_n=0):
        """the decoder's steps penalise the ids at positions [max(start, n - last_n), n) of its own ids from now on ((1, 0, 0): off;
        last_n 0: no limit; include/gten_host_penalty.h)"""
        rc = self.set_penalty_rc(rep, freq, pres, start, last_n)
        if rc:
            raise GtenHipError(f"set_penalty rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def penalty_info(self):
        """(rep, freq, pres, start, last_n, whether the decoder has ever had a penalty set)"""
        r, f, p, s, l = np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        on = self.host._m_pen_info(self.h, _ptr(r), _ptr(f), _ptr(p), _ptr(s), _ptr(l))
        if on < 0:
            raise GtenHipError(f"penalty_info rc={on}")
        return r[0], f[0], p[0], int(s[0]), int(l[0]), bool(on)

    def generate_penalized(self, prompt, max_tokens, eos=-1, top_k=0, temp=1.0, seed=0, stream=0, rep=1.0, freq=0.0, pres=0.0, last_n=0,
                           count_prompt=True, top_p=1.0, min_p=0.0, table=-1, min_new=0, n_top=None):
        """generate_nucleus() with the ids the sequence already holds penalised (include/gten_host_penalty.h): rep divides a positive
        logit (multiplies a negative one), freq is subtracted per occurrence, pres once; over the last last_n positions (0: all), the
        prompt's included or not.  top_k 0: penalised greedy."""
        width = max(max_tokens, len(prompt))
        buf = np.zeros(width, np.int32)
        buf[: len(prompt)] = prompt
        ask = n_top is not None and n_top >= 0
        w = int(n_top) if ask else 0
        lp, ti, tl = np.zeros(width, np.float32), np.full((width, w), -1, np.int32), np.zeros((width, w), np.float32)
        pen = _penalty_arg(1, float(rep), float(freq), float(pres), int(last_n), bool(count_prompt))
        total = self.host._generate_pen(self.h, _ptr(buf), len(prompt), max_tokens, eos, int(top_k), float(temp), C.c_uint64(int(seed)),
                                        C.c_uint32(int(stream)), int(table), int(min_new), w if ask else -1, C.c_float(top_p), C.c_float(min_p),
                                        _ptr(lp) if ask else None, _ptr(ti) if ask else None, _ptr(tl) if ask else None, C.byref(pen))
        if total < 0:
            raise GtenHipError(f"generate_penalized rc={total}: {self.host.hip._err().decode(errors='replace')}")
        ids = buf[:total].copy()
        return (ids, lp[:total].copy(), ti[:total].copy(), tl[:total].copy()) if ask else ids

    # ---- context shift (include/gten_host_shift.h)
    def generate_shifting_rc(self, prompt, max_tokens, keep, drop=0, eos=-1, top_k=0, temp=1.0, seed=0, stream=0, rep=1.0, freq=0.0, pres=0.0, last_n=0,
                             count_prompt=True, top_p=1.0, min_p=0.0, table=-1, n_top=None):
        """gten_host_model_generate_shifting: (total or a negative code, ids)"""
        width = max(max_tokens, len(prompt))
        buf = np.zeros(width, np.int32)
        buf[: len(prompt)] = prompt
        pen = _penalty_arg(1, float(rep), float(freq), float(pres), int(last_n), bool(count_prompt))
        total = self.host._generate_shift(self.h, _ptr(buf), len(prompt), max_tokens, eos, int(top_k), float(temp), C.c_uint64(int(seed)),
                                          C.c_uint32(int(stream)), int(table), -1 if n_top is None else int(n_top), C.c_float(top_p), C.c_float(min_p),
                                          C.byref(pen), int(keep), int(drop))
        return total, buf[: max(total, 0)].copy()

    def generate_shifting(self, prompt, max_tokens, keep, drop=0, **requests):
        """generate_penalized() that goes on past the window: whenever it is full the caches are shifted by (keep, drop) -- drop 0: half
        of what lies behind keep -- and generation continues; max_tokens may exceed max_ctx, the ids come back in generation order.
        keep < 0: generate_penalized() itself."""
        total, ids = self.generate_shifting_rc(prompt, max_tokens, keep, drop, **requests)
        if total < 0:
            raise GtenHipError(f"generate_shifting rc={total}: {self.host.shift_error() or self.host.hip._err().decode(errors='replace')}")
        return ids

    def shift(self, n_rows, keep, drop=0):
        """gten_host_model_shift: this model's caches, n_rows of them valid, shifted by (keep, drop)"""
        rc = self.host._mshift(self.h, int(n_rows), int(keep), int(drop))
        if rc:
            raise GtenHipError(f"model_shift rc={rc}: {self.host.shift_error() or self.host.hip._err().decode(errors='replace')}")

    def shift_info(self):
        """(shifts done, rows moved, rows dropped)"""
        u = [C.c_ulonglong(0) for _ in range(3)]
        self.host._mshift_info(self.h, *[C.byref(x) for x in u])
        return tuple(x.value for x in u)

    def set_fsm_rc(self, fsm):
        return self.host._m_set_fsm(self.h, fsm.h if fsm is not None else None)

    def set_fsm(self, fsm):
        """the decoder's automaton pool becomes `fsm` (an Fsm; None drops it; include/gten_host_fsm.h)"""
        rc = self.set_fsm_rc(fsm)
        if rc:
            raise GtenHipError(f"set_fsm rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def set_mirostat_rc(self, tau, eta=0.1, mu_q16=None, pos=0):
        return self.host._m_set_mirostat(self.h, C.c_float(tau), C.c_float(eta), int(MIRO_MU_DEFAULT if mu_q16 is None else mu_q16), int(pos))

    def set_mirostat(self, tau, eta=0.1, mu_q16=None, pos=0):
        """the ids from position pos on are drawn under Mirostat v2 (tau, eta), mu starting at mu_q16 (Q16; None: 2 tau); tau 0 unbinds"""
        rc = self.set_mirostat_rc(tau, eta, mu_q16, pos)
        if rc:
            raise GtenHipError(f"set_mirostat rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def mirostat_info(self):
        """(tau_q int32[1], eta_q int32[1], binding position int32[1], whether a sequence was ever bound)"""
        return _mirostat_info(self.host._m_mirostat_info, self.h, 1)

    def mirostat_mus(self, n_from, count):
        """entries [n_from, n_from + count) of the sequence's mu row (Q16)"""
        out = np.zeros(max(count, 1), np.int32)
        rc = self.host._m_mirostat_mus(self.h, int(n_from), int(count), _ptr(out))
        if rc:
            raise GtenHipError(f"mirostat_mus rc={rc}: {self.host.hip._err().decode(errors='replace')}")
        return out[:count].copy()

    def fsm_info(self):
        """(states of the decoder's pool, binding state int32[1], binding position int32[1], whether a sequence was ever bound)"""
        return _fsm_info(self.host._m_fsm_info, self.h, 1)

    def set_seq_fsm_rc(self, state, pos=0):
        return self.host._m_set_seq_fsm(self.h, int(state), int(pos))

    def set_seq_fsm(self, state, pos=0):
        """the id at position pos is chosen in `state` of the decoder's pool from now on (-1: unbound)"""
        rc = self.set_seq_fsm_rc(state, pos)
        if rc:
            raise GtenHipError(f"set_seq_fsm rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def fsm_states(self, n_from, count):
        """entries [n_from, n_from + count) of the sequence's state row"""
        out = np.zeros(max(count, 1), np.int32)
        rc = self.host._m_fsm_states(self.h, int(n_from), int(count), _ptr(out))
        if rc:
            raise GtenHipError(f"fsm_states rc={rc}: {self.host.hip._err().decode(errors='replace')}")
        return out[:count].copy()

    def generate_fsm(self, prompt, max_tokens, fsm_start, eos=-1, top_k=0, temp=1.0, seed=0, stream=0, rep=1.0, freq=0.0, pres=0.0, last_n=0,
                     count_prompt=True, top_p=1.0, min_p=0.0, n_top=None):
        """generate_penalized() with the first new id chosen in state fsm_start of the decoder's pool (-1: not bound): (ids, ended_by)
        -- ended_by 0 length or context, 1 eos, 2 a final state -- or with n_top (ids, ended_by, lp, top ids, top lps)"""
        width = max(max_tokens, len(prompt))
        buf = np.zeros(width, np.int32)
        buf[: len(prompt)] = prompt
        ask = n_top is not None and n_top >= 0
        w = int(n_top) if ask else 0
        lp, ti, tl = np.zeros(width, np.float32), np.full((width, w), -1, np.int32), np.zeros((width, w), np.float32)
        pen = _penalty_arg(1, float(rep), float(freq), float(pres), int(last_n), bool(count_prompt))
        ended = np.zeros(1, np.int32)
        total = self.host._generate_fsm(self.h, _ptr(buf), len(prompt), max_tokens, eos, int(top_k), float(temp), C.c_uint64(int(seed)),
                                        C.c_uint32(int(stream)), -1, 0, w if ask else -1, C.c_float(top_p), C.c_float(min_p),
                                        _ptr(lp) if ask else None, _ptr(ti) if ask else None, _ptr(tl) if ask else None, C.byref(pen), int(fsm_start),
                                        _ptr(ended))
        if total < 0:
            raise GtenHipError(f"generate_fsm rc={total}: {self.host.hip._err().decode(errors='replace')}")
        ids = buf[:total].copy()
        return (ids, int(ended[0]), lp[:total].copy(), ti[:total].copy(), tl[:total].copy()) if ask else (ids, int(ended[0]))

    def generate_mirostat(self, prompt, max_tokens, tau, eta=0.1, eos=-1, top_k=40, temp=1.0, seed=0, stream=0, rep=1.0, freq=0.0, pres=0.0, last_n=0,
                          count_prompt=True, top_p=1.0, min_p=0.0, table=-1, min_new=0, fsm_start=-1):
        """generate_fsm() under Mirostat v2 (include/gten_host_mirostat.h): the surprise of the new ids is held at tau bits with learning
        rate eta (tau 0: off).  Returns the ids.  A cut beside Mirostat is refused."""
        width = max(max_tokens, len(prompt))
        buf = np.zeros(width, np.int32)
        buf[: len(prompt)] = prompt
        pen = _penalty_arg(1, float(rep), float(freq), float(pres), int(last_n), bool(count_prompt))
        ended = np.zeros(1, np.int32)
        total = self.host._generate_miro(self.h, _ptr(buf), len(prompt), max_tokens, eos, int(top_k), float(temp), C.c_uint64(int(seed)),
                                         C.c_uint32(int(stream)), int(table), int(min_new), -1, C.c_float(top_p), C.c_float(min_p), None, None, None,
                                         C.byref(pen), int(fsm_start), _ptr(ended), C.c_float(tau), C.c_float(eta))
        if total < 0:
            raise GtenHipError(f"generate_mirostat rc={total}: {self.host.hip._err().decode(errors='replace')}")
        return buf[:total].copy()

    def generate_regex(self, prompt, max_tokens, pattern, vocab, eos=-1, **kw):
        """generate_fsm() bound to `pattern` (None: not bound): a pool of that one pattern over `vocab` (what Fsm.set_vocab takes) becomes
        the decoder's pool -- expanded on the device -- and the first new id is chosen in its start state.  kw: generate_fsm's."""
        if pattern is None:
            return self.generate_fsm(prompt, max_tokens, -1, eos, **kw)
        f = Fsm(self.host, self.cfg.n_vocab)
        try:
            f.set_vocab(vocab)
            start = f.add_regex(pattern, eos)
            self.set_fsm(f)
            return self.generate_fsm(prompt, max_tokens, start, eos, **kw)
        finally:
            f.close()

    def generate_stop_text(self, prompt, max_tokens, strings, vocab, eos=-1, **kw):
        """generate_fsm() that ends at the first of `strings` (str / bytes; None or empty: not bound) in the NEW text: a pool of that one
        search range over `vocab` (what Fsm.set_vocab takes) becomes the decoder's pool, expanded on the device.  Nothing is banned; the
        id that completes a string is kept.  Returns (ids, ended_by, new text as bytes, cut before the string).  kw: generate_fsm's."""
        f = Fsm(self.host, self.cfg.n_vocab)
        try:
            f.set_vocab(vocab)
            start = -1
            if strings:
                start = f.add_stop_text(strings)
                self.set_fsm(f)
            ids, ended = self.generate_fsm(prompt, max_tokens, start, eos, **kw)[:2]
            return ids, ended, _cut_text(self.host, f.vocab, ids[len(prompt):], strings)
        finally:
            f.close()

    def generate_json(self, prompt, max_tokens, schema, vocab, eos, ws=0, depth=2, **kw):
        """generate_regex() of json_schema_regex(schema, ws, depth): the new text is a JSON document that fits the schema, ended by its
        last byte where nothing can follow (ended_by 2), else by eos"""
        return self.generate_regex(prompt, max_tokens, json_schema_regex(self.host, schema, ws, depth), vocab, eos, **kw)

    def close(self):
        if self.h:
            self.host._free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBatch:
    """n_seq sequences sharing one copy of the weights; one step advances all of them."""

    def __init__(self, host, cfg, n_seq):
        self.host, self.cfg, self.n_seq = host, cfg, n_seq
        if host.hip.device_count() < 1:
            raise GtenHipError("no MI355X visible: the model runs only on the gten_hip path")
        self.h = host._bcreate(C.byref(cfg), n_seq)
        if not self.h:
            raise GtenHipError(f"batch_create(n_seq={n_seq}) failed")

    def _ck(self, rc, what):
        if rc:
            raise GtenHipError(f"{what} rc={rc}")

    def load_synthetic(self, seed):
        self._ck(self.host._bloads(self.h, seed), "batch_load_synthetic")

    def set_weight(self, idx, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self._ck(self.host._bsetw(self.h, idx, data.ctypes.data_as(C.c_void_p), data.size), f"batch_set_weight({idx})")

    def prefill(self, seq, tokens, want=True):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.zeros(self.cfg.n_vocab, np.float32) if want else None
        self._ck(self.host._bprefill(self.h, seq, tokens.ctypes.data_as(C.c_void_p), len(tokens),
                                     out.ctypes.data_as(C.c_void_p) if want else None), "batch_prefill")
        return out

    def prefill_many(self, seqs, prompts, want=True):
        """several prompts (>= 16 ids each) as segments of one row matrix, prompt k onto the caches of sequence seqs[k];
        returns [n_prompts][n_vocab] logits (wide batches only: raises otherwise)"""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        starts = np.zeros(len(prompts) + 1, np.int32)
        starts[1:] = np.cumsum([len(p) for p in prompts])
        toks = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32) for p in prompts]), dtype=np.int32)
        out = np.zeros((len(prompts), self.cfg.n_vocab), np.float32) if want else None
        self._ck(self.host._bprefill_many(self.h, seqs.ctypes.data_as(C.c_void_p), toks.ctypes.data_as(C.c_void_p), starts.ctypes.data_as(C.c_void_p),
                                          len(prompts), out.ctypes.data_as(C.c_void_p) if want else None), "batch_prefill_many")
        return out

    def extend_many_rc(self, seqs, ctx_len, tails, out=None, first=None):
        """gten_host_batch_extend_many's return code (tests: the refusals)"""
        seqs = np.ascontiguousarray(seqs, dtype=np.int32)
        ctx_len = np.ascontiguousarray(ctx_len, dtype=np.int32)
        starts = np.zeros(len(tails) + 1, np.int32)
        starts[1:] = np.cumsum([len(t) for t in tails])
        toks = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32) for t in tails] + [np.zeros(1, np.int32)]), dtype=np.int32)
        return self.host._bextend_many(self.h, seqs.ctypes.data_as(C.c_void_p), ctx_len.ctypes.data_as(C.c_void_p), toks.ctypes.data_as(C.c_void_p),
                                       starts.ctypes.data_as(C.c_void_p), len(tails), out.ctypes.data_as(C.c_void_p) if out is not None else None,
                                       first.ctypes.data_as(C.c_void_p) if first is not None else None)

    def extend_many(self, seqs, ctx_len, tails, want=True):
        """sequence seqs[k] keeps rows [0, ctx_len[k]) of its caches, tails[k] become positions ctx_len[k] .. (include/gten_host_sessions.h):
        only the new rows are computed.  Returns ([n][n_vocab] logits of the segments' last rows or None, their argmax ids)"""
        out = np.zeros((len(tails), self.cfg.n_vocab), np.float32) if want else None
        first = np.zeros(len(tails), np.int32)
        self._ck(self.extend_many_rc(seqs, ctx_len, tails, out, first), "batch_extend_many")
        return out, first

    def extend_info(self):
        """(segments that went as continued row matrices, rows computed for them, context rows kept, rows of one-by-one segments)"""
        a, b, c, d = (C.c_ulonglong(0) for _ in range(4))
        self._ck(self.host._bextend_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "batch_extend_info")
        return a.value, b.value, c.value, d.value

    def decode_begin(self, seq, tokens):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        self._ck(self.host._bbegin(self.h, seq, tokens.ctypes.data_as(C.c_void_p), len(tokens)), "batch_decode_begin")

    def decode_step(self, n, use_graph=True):
        self._ck(self.host._bstep(self.h, n, 1 if use_graph else 0), f"batch_decode_step({n})")

    def decode_steps(self, n_first, count, use_graph=True):
        self._ck(self.host._bsteps(self.h, n_first, count, 1 if use_graph else 0), f"batch_decode_steps({n_first}, {count})")

    def decode_step_ragged(self, ns, use_graph=True):
        """sequence q decodes row ns[q] - 1 (continuous batching)"""
        ns = np.ascontiguousarray(ns, dtype=np.int32)
        assert len(ns) == self.n_seq
        self._ck(self.host._bstepr(self.h, ns.ctypes.data_as(C.c_void_p), 1 if use_graph else 0), "batch_decode_step_ragged")

    def _generate(self, fn, what, prompts, max_tokens, eos, requests=(), records=()):
        """one fixed-batch entry point: fn(handle, prompts, lengths, longest, max_tokens, eos, *requests, ids out, totals out, *records)"""
        assert len(prompts) == self.n_seq
        pr, npr, mp = _pack(prompts)
        out, tot = np.zeros((self.n_seq, max_tokens), np.int32), np.zeros(self.n_seq, np.int32)
        self._ck(fn(self.h, _ptr(pr), _ptr(npr), mp, max_tokens, eos, *requests, _ptr(out), _ptr(tot), *records), what)
        return [out[q, : tot[q]].copy() for q in range(self.n_seq)]

    def _serve(self, fn, what, prompts, max_tokens, eos, slice_steps, max_new, max_new_each, *extra):
        """one serve entry point: gten_host_batch_serve2's arguments, then `extra`; returns (ids per prompt, the stats dict)"""
        n = len(prompts)
        pr, npr, mp = _pack(prompts)
        out, tot, st = np.zeros((n, max(max_tokens, mp)), np.int32), np.zeros(n, np.int32), np.zeros(len(SERVE_STATS), np.float64)
        each, _ = _each(max_new_each, n, np.int32)
        self._ck(fn(self.h, _ptr(pr), _ptr(npr), n, mp, max_tokens, eos, slice_steps, max_new, _ptr(each), _ptr(out), _ptr(tot), _ptr(st), len(st), *extra), what)
        return [out[j, : tot[j]].copy() for j in range(n)], dict(zip(SERVE_STATS, st.tolist()))

    def generate(self, prompts, max_tokens, eos=-1):
        """greedy generation of every sequence (sampler on the device): list of id arrays, one per sequence, prompt included"""
        return self._generate(self.host._bgen, "batch_generate", prompts, max_tokens, eos)

    def generate_topk(self, prompts, max_tokens, eos, top_k, temp, seed, streams=None):
        """generate() with every new id drawn by the device sampler; sequence q uses streams[q] (None: q)"""
        st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
        return self._generate(self.host._bgen_topk, "batch_generate_topk", prompts, max_tokens, eos,
                              [int(top_k), float(temp), C.c_uint64(int(seed)), _ptr(st)])

    def set_serve_schedule(self, k):
        """tests: exactly k prompts beside every slice (0: as many as fit while it runs)"""
        self._ck(self.host._bsched(self.h, int(k)), "set_serve_schedule")

    def set_serve_spares(self, n):
        """cache sets that serve() fills ahead of the slots that will take them (-1: default, 0: none)"""
        self._ck(self.host._bspares(self.h, int(n)), "set_serve_spares")

    def set_serve_ramp(self, percent):
        """percent of the slots that get a processed prompt before a queue's first slice starts (default 100)"""
        self._ck(self.host._bramp(self.h, int(percent)), "set_serve_ramp")

    def serve(self, prompts, max_tokens, eos=-1, slice_steps=16, max_new=0, max_new_each=None):
        """continuous batching: the queue `prompts` (any number) through this batch's slots; returns (list of id
        arrays -- prompt + new ids, one per prompt, in queue order -- and a dict of counters)"""
        return self._serve(self.host._bserve, "batch_serve", prompts, max_tokens, eos, slice_steps, max_new, max_new_each)

    def serve_topk(self, prompts, max_tokens, eos, top_k, temp, seed, slice_steps=16, max_new=0, max_new_each=None):
        """serve() with every new id drawn by the device sampler: top_k / temp a scalar or one value per prompt (top_k 0: greedy),
        prompt j draws with stream j"""
        return self._serve(self.host._bserve_topk, "batch_serve_topk", prompts, max_tokens, eos, slice_steps, max_new, max_new_each,
                           *_request_args(len(prompts), top_k, temp, seed))

    def set_bias_table_rc(self, table, pairs=(), fill=0.0, allow=None):
        """gten_host_batch_set_bias_table's return code (0, or the refusal: the table keeps its contents)"""
        ids, values, fill = bias_pairs(pairs, fill, allow)
        return self.host._b_bias_table(self.h, int(table), ids.ctypes.data_as(C.c_void_p), values.ctypes.data_as(C.c_void_p), len(ids), C.c_float(fill))

    def set_bias_table(self, table, pairs=(), fill=0.0, allow=None):
        """bias table `table` of the shared decoder := fill everywhere, then value at id for (id, value) in pairs; allow=[ids]: only
        these ids (include/gten_host_bias.h)"""
        rc = self.set_bias_table_rc(table, pairs, fill, allow)
        if rc:
            raise GtenHipError(f"batch_set_bias_table rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def set_sampling(self, seq, top_k, temp=1.0, seed=0, stream=0):
        """sequence seq's request for the steps the caller drives (decode_step): top_k 0 = greedy"""
        self._ck(self.host._b_set_sampling(self.h, int(seq), int(top_k), float(temp), C.c_uint64(int(seed)), C.c_uint32(int(stream))), "batch_set_sampling")

    def set_seq_bias_rc(self, seq, table, until=0):
        return self.host._b_seq_bias(self.h, int(seq), int(table), int(until))

    def set_seq_bias(self, seq, table, until=0):
        """sequence seq draws under `table` at positions < until (0: always); table -1 clears it"""
        self._ck(self.set_seq_bias_rc(seq, table, until), "batch_set_seq_bias")

    def bias_info(self):
        """(number of tables, table per sequence [-1: none], until per sequence)"""
        t, u = np.zeros(self.n_seq, np.int32), np.zeros(self.n_seq, np.int32)
        n = self.host._b_bias_info(self.h, t.ctypes.data_as(C.c_void_p), u.ctypes.data_as(C.c_void_p))
        if n < 0:
            raise GtenHipError(f"batch_bias_info rc={n}")
        return n, t, u

    def generate_biased(self, prompts, max_tokens, eos=-1, top_k=0, temp=1.0, seed=0, streams=None, tables=None, min_new=None):
        """generate_topk() with a request per sequence: top_k / temp a scalar or a list, tables[q] (-1 / None: no table) and
        min_new[q] (0 / None: the table holds throughout)"""
        n = self.n_seq
        return self._generate(self.host._bgen_biased, "batch_generate_biased", prompts, max_tokens, eos,
                              _request_args(n, top_k, temp, seed) + _full_args(n, (streams, np.uint32), (tables, np.int32), (min_new, np.int32)))

    def serve_biased(self, prompts, max_tokens, eos, top_k, temp, seed, tables=None, min_new=None, slice_steps=16, max_new=0, max_new_each=None):
        """serve_topk() with a bias table (-1: none) and a min_new (0: the table holds throughout) per prompt"""
        n = len(prompts)
        return self._serve(self.host._bserve_biased, "batch_serve_biased", prompts, max_tokens, eos, slice_steps, max_new, max_new_each,
                           *_request_args(n, top_k, temp, seed), *_full_args(n, (tables, np.int32), (min_new, np.int32)))

    def set_logprobs_rc(self, seq, n_top):
        return self.host._b_set_lp(self.h, int(seq), int(n_top))

    def set_logprobs(self, seq, n_top):
        """sequence seq's steps commit a log-prob record with n_top alternatives from now on (-1: off; include/gten_host_logprobs.h)"""
        rc = self.set_logprobs_rc(seq, n_top)
        if rc:
            raise GtenHipError(f"batch_set_logprobs rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def logprobs(self, seq, n_from, count, n_top):
        """(logprob f32[count], top_id int32[count][n_top], top_logprob f32[count][n_top]) of sequence seq's positions [n_from, n_from + count)"""
        lp, ti, tl = np.zeros(count, np.float32), np.full((count, n_top), -1, np.int32), np.zeros((count, n_top), np.float32)
        rc = self.host._b_lp(self.h, int(seq), int(n_from), int(count), int(n_top), lp.ctypes.data_as(C.c_void_p), ti.ctypes.data_as(C.c_void_p),
                             tl.ctypes.data_as(C.c_void_p))
        if rc:
            raise GtenHipError(f"batch_logprobs rc={rc}: {self.host.hip._err().decode(errors='replace')}")
        return lp, ti, tl

    def generate_logprobs(self, prompts, max_tokens, n_top, eos=-1, top_k=0, temp=1.0, seed=0, streams=None, tables=None, min_new=None):
        """generate_biased() plus the records of the sequences that ask (n_top a scalar or a list, -1 / None: not this one): returns
        (ids per sequence, logprob [n_seq][max_tokens], top_id [n_seq][max_tokens][max n_top], top_logprob), aligned with the ids"""
        n = self.n_seq
        args, rec = _records(n_top, n, max_tokens)
        ids = self._generate(self.host._bgen_lp, "batch_generate_lp", prompts, max_tokens, eos,
                             _request_args(n, top_k, temp, seed) + _full_args(n, (streams, np.uint32), (tables, np.int32), (min_new, np.int32)), args)
        return (ids, *rec)

    def serve_logprobs(self, prompts, max_tokens, eos, top_k, temp, seed, n_top, tables=None, min_new=None, slice_steps=16, max_new=0,
                       max_new_each=None):
        """serve_biased() plus the records of the prompts that ask (n_top per prompt, -1 / None: not this one): returns
        (ids per prompt, stats, logprob [n][width], top_id [n][width][max n_top], top_logprob), width = max(max_tokens, longest prompt)"""
        n = len(prompts)
        args, rec = _records(n_top, n, max(max_tokens, max(len(p) for p in prompts)))
        ids, st = self._serve(self.host._bserve_lp, "batch_serve_lp", prompts, max_tokens, eos, slice_steps, max_new, max_new_each,
                              *_request_args(n, top_k, temp, seed), *_full_args(n, (tables, np.int32), (min_new, np.int32)), *args)
        return (ids, st, *rec)

    def set_cut_rc(self, seq, top_p, min_p):
        return self.host._b_set_cut(self.h, int(seq), C.c_float(top_p), C.c_float(min_p))

    def set_cut(self, seq, top_p=1.0, min_p=0.0):
        """sequence seq's sampled steps draw under the cut (top_p, min_p) from now on ((1, 0): off; include/gten_host_nucleus.h)"""
        rc = self.set_cut_rc(seq, top_p, min_p)
        if rc:
            raise GtenHipError(f"batch_set_cut rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def resident(self):
        """HostModel.resident() of the shared decoder: a decoder of 2+ sequences keeps no weights resident"""
        return self.host._resident_of(self.host._b_resident, self.h)

    def o_planes(self):
        """HostModel.o_planes() of the shared decoder: a decoder of 2+ sequences keeps the one-plane launch"""
        return self.host._o_planes_of(self.host._b_o_planes, self.h)

    def cut_info(self):
        """(top_p f32[n_seq], min_p f32[n_seq], t f32[n_seq] = f32(log(min_p)), whether the shared decoder has ever had a cut set)"""
        a, b, t = np.zeros(self.n_seq, np.float32), np.zeros(self.n_seq, np.float32), np.zeros(self.n_seq, np.float32)
        on = self.host._b_cut_info(self.h, _ptr(a), _ptr(b), _ptr(t))
        if on < 0:
            raise GtenHipError(f"batch_cut_info rc={on}")
        return a, b, t, bool(on)

    def generate_nucleus(self, prompts, max_tokens, eos=-1, top_k=0, temp=1.0, seed=0, streams=None, top_p=1.0, min_p=0.0, tables=None,
                         min_new=None, n_top=None):
        """generate_biased() with a cut per sequence (top_p / min_p a scalar or a list); n_top None: the ids per sequence, otherwise
        generate_logprobs()'s tuple"""
        n = self.n_seq
        args, rec = _records(n_top, n, max_tokens)
        if n_top is None:
            args = [None, 0, None, None, None]
        ids = self._generate(self.host._bgen_nuc, "batch_generate_nucleus", prompts, max_tokens, eos,
                             _request_args(n, top_k, temp, seed) + _full_args(n, (streams, np.uint32), (tables, np.int32), (min_new, np.int32)),
                             args + _cut_args(n, top_p, min_p))
        return ids if n_top is None else (ids, *rec)

    def serve_nucleus(self, prompts, max_tokens, eos, top_k, temp, seed, top_p=1.0, min_p=0.0, tables=None, min_new=None, n_top=None,
                      slice_steps=16, max_new=0, max_new_each=None):
        """serve_biased() with a cut per prompt; n_top None: (ids per prompt, stats), otherwise serve_logprobs()'s tuple"""
        n = len(prompts)
        args, rec = _records(n_top, n, max(max_tokens, max(len(p) for p in prompts)))
        if n_top is None:
            args = [None, 0, None, None, None]
        ids, st = self._serve(self.host._bserve_nuc, "batch_serve_nucleus", prompts, max_tokens, eos, slice_steps, max_new, max_new_each,
                              *_request_args(n, top_k, temp, seed), *_full_args(n, (tables, np.int32), (min_new, np.int32)), *args,
                              *_cut_args(n, top_p, min_p))
        return (ids, st) if n_top is None else (ids, st, *rec)

    def set_penalty_rc(self, seq, rep, freq=0.0, pres=0.0, start=0, last_n=0):
        return self.host._b_set_pen(self.h, int(seq), C.c_float(rep), C.c_float(freq), C.c_float(pres), int(start), int(last_n))

    def set_penalty(self, seq, rep=1.0, freq=0.0, pres=0.0, start=0, last_n=0):
        """sequence seq's steps penalise the ids at positions [max(start, n - last_n), n) of its own ids from now on ((1, 0, 0): off;
        include/gten_host_penalty.h)"""
        rc = self.set_penalty_rc(seq, rep, freq, pres, start, last_n)
        if rc:
            raise GtenHipError(f"batch_set_penalty rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def penalty_info(self):
        """(rep f32[n_seq], freq, pres, start int32[n_seq], last_n, whether the shared decoder has ever had a penalty set)"""
        n = self.n_seq
        r, f, p, s, l = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        on = self.host._b_pen_info(self.h, _ptr(r), _ptr(f), _ptr(p), _ptr(s), _ptr(l))
        if on < 0:
            raise GtenHipError(f"batch_penalty_info rc={on}")
        return r, f, p, s, l, bool(on)

    def generate_penalized(self, prompts, max_tokens, eos=-1, top_k=0, temp=1.0, seed=0, streams=None, rep=1.0, freq=0.0, pres=0.0, last_n=0,
                           count_prompt=True, top_p=1.0, min_p=0.0, tables=None, min_new=None, n_top=None):
        """generate_nucleus() with a penalty per sequence (rep / freq / pres / last_n / count_prompt a scalar or a list)"""
        n = self.n_seq
        args, rec = _records(n_top, n, max_tokens)
        if n_top is None:
            args = [None, 0, None, None, None]
        pen = _penalty_arg(n, rep, freq, pres, last_n, count_prompt)
        ids = self._generate(self.host._bgen_pen, "batch_generate_penalized", prompts, max_tokens, eos,
                             _request_args(n, top_k, temp, seed) + _full_args(n, (streams, np.uint32), (tables, np.int32), (min_new, np.int32)),
                             args + _cut_args(n, top_p, min_p) + [C.byref(pen)])
        return ids if n_top is None else (ids, *rec)

    def serve_penalized(self, prompts, max_tokens, eos, top_k, temp, seed, rep=1.0, freq=0.0, pres=0.0, last_n=0, count_prompt=True, top_p=1.0,
                        min_p=0.0, tables=None, min_new=None, n_top=None, slice_steps=16, max_new=0, max_new_each=None):
        """serve_nucleus() with a penalty per prompt; n_top None: (ids per prompt, stats), otherwise serve_logprobs()'s tuple"""
        n = len(prompts)
        args, rec = _records(n_top, n, max(max_tokens, max(len(p) for p in prompts)))
        if n_top is None:
            args = [None, 0, None, None, None]
        pen = _penalty_arg(n, rep, freq, pres, last_n, count_prompt)
        ids, st = self._serve(self.host._bserve_pen, "batch_serve_penalized", prompts, max_tokens, eos, slice_steps, max_new, max_new_each,
                              *_request_args(n, top_k, temp, seed), *_full_args(n, (tables, np.int32), (min_new, np.int32)), *args,
                              *_cut_args(n, top_p, min_p), C.byref(pen))
        return (ids, st) if n_top is None else (ids, st, *rec)

    def set_fsm_rc(self, fsm):
        return self.host._b_set_fsm(self.h, fsm.h if fsm is not None else None)

    def set_fsm(self, fsm):
        """the shared decoder's automaton pool becomes `fsm` (an Fsm; None drops it; include/gten_host_fsm.h)"""
        rc = self.set_fsm_rc(fsm)
        if rc:
            raise GtenHipError(f"batch_set_fsm rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def set_mirostat_rc(self, seq, tau, eta=0.1, mu_q16=None, pos=0):
        return self.host._b_set_mirostat(self.h, int(seq), C.c_float(tau), C.c_float(eta), int(MIRO_MU_DEFAULT if mu_q16 is None else mu_q16), int(pos))

    def set_mirostat(self, seq, tau, eta=0.1, mu_q16=None, pos=0):
        """sequence seq's ids from position pos on are drawn under Mirostat v2 (tau, eta), mu starting at mu_q16 (Q16; None: 2 tau); tau 0 unbinds"""
        rc = self.set_mirostat_rc(seq, tau, eta, mu_q16, pos)
        if rc:
            raise GtenHipError(f"batch_set_mirostat rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def mirostat_info(self):
        """(tau_q int32[n_seq], eta_q int32[n_seq], binding position int32[n_seq], whether one was ever bound)"""
        return _mirostat_info(self.host._b_mirostat_info, self.h, self.n_seq)

    def mirostat_mus(self, seq, n_from, count):
        """entries [n_from, n_from + count) of sequence seq's mu row (Q16)"""
        out = np.zeros(max(count, 1), np.int32)
        rc = self.host._b_mirostat_mus(self.h, int(seq), int(n_from), int(count), _ptr(out))
        if rc:
            raise GtenHipError(f"batch_mirostat_mus rc={rc}: {self.host.hip._err().decode(errors='replace')}")
        return out[:count].copy()

    def fsm_info(self):
        """(states of the shared decoder's pool, binding state int32[n_seq], binding position int32[n_seq], whether one was ever bound)"""
        return _fsm_info(self.host._b_fsm_info, self.h, self.n_seq)

    def set_seq_fsm_rc(self, seq, state, pos=0):
        return self.host._b_set_seq_fsm(self.h, int(seq), int(state), int(pos))

    def set_seq_fsm(self, seq, state, pos=0):
        """the id at position pos of sequence seq is chosen in `state` of the shared decoder's pool from now on (-1: unbound)"""
        rc = self.set_seq_fsm_rc(seq, state, pos)
        if rc:
            raise GtenHipError(f"batch_set_seq_fsm rc={rc}: {self.host.hip._err().decode(errors='replace')}")

    def fsm_states(self, seq, n_from, count):
        """entries [n_from, n_from + count) of sequence seq's state row"""
        out = np.zeros(max(count, 1), np.int32)
        rc = self.host._b_fsm_states(self.h, int(seq), int(n_from), int(count), _ptr(out))
        if rc:
            raise GtenHipError(f"batch_fsm_states rc={rc}: {self.host.hip._err().decode(errors='replace')}")
        return out[:count].copy()

    def fsm_decoder(self):
        """the shared decoder's raw handle, for hipabi's decoder_slot_* calls"""
        return self.host._b_fsm_decoder(self.h)

    def beam_search_rc(self, prompts, n_beams, max_new, eos=-1, length_penalty=1.0):
        """gten_host_batch_beam_search: (return code, hypotheses per prompt or None, rounds run)"""
        G = len(prompts)
        starts = np.zeros(G + 1, np.int32)
        starts[1:] = np.cumsum([len(p) for p in prompts])
        toks = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32) for p in prompts]), dtype=np.int32)
        nb = max(int(n_beams), 1)
        oi, on = np.zeros((G, nb, max(max_new, 1)), np.int32), np.zeros((G, nb), np.int32)
        of, oc, oe = np.zeros((G, nb), np.float32), np.zeros((G, nb), np.float32), np.zeros((G, nb), np.int32)
        nh, rounds = np.zeros(G, np.int32), C.c_int(0)
        rc = self.host._bbeam(self.h, _ptr(toks), _ptr(starts), G, int(n_beams), int(max_new), int(eos), float(length_penalty), _ptr(oi), _ptr(on), _ptr(of),
                              _ptr(oc), _ptr(oe), _ptr(nh), C.byref(rounds))
        if rc:
            return rc, None, rounds.value
        return 0, [[(oi[g, i, : on[g, i]].copy(), of[g, i], oc[g, i], GtenHost.BEAM_ENDED[oe[g, i]]) for i in range(nh[g])] for g in range(G)], rounds.value

    def beam_search(self, prompts, n_beams, max_new, eos=-1, length_penalty=1.0):
        """beam search (include/gten_host_beam.h): prompt g x n_beams beams on sequences g * n_beams + b.  Per prompt a list of
        (new ids, final, cum, ended_by 'eos' | 'length'), best first"""
        rc, out, _ = self.beam_search_rc(prompts, n_beams, max_new, eos, length_penalty)
        self._ck(rc, "batch_beam_search")
        return out

    def generate_fsm(self, prompts, max_tokens, fsm_start, eos=-1, top_k=0, temp=1.0, seed=0, streams=None, rep=1.0, freq=0.0, pres=0.0, last_n=0,
                     count_prompt=True, top_p=1.0, min_p=0.0, tables=None, min_new=None):
        """generate_penalized() with a start state per sequence (a scalar for all; -1: not bound): (ids per sequence, ended_by int32[n_seq])"""
        n = self.n_seq
        pen = _penalty_arg(n, rep, freq, pres, last_n, count_prompt)
        st, ended = np.ascontiguousarray(np.broadcast_to(np.asarray(fsm_start, np.int32), (n,))), np.zeros(n, np.int32)
        ids = self._generate(self.host._bgen_fsm, "batch_generate_fsm", prompts, max_tokens, eos,
                             _request_args(n, top_k, temp, seed) + _full_args(n, (streams, np.uint32), (tables, np.int32), (min_new, np.int32)),
                             [None, 0, None, None, None] + _cut_args(n, top_p, min_p) + [C.byref(pen), _ptr(st), _ptr(ended)])
        return ids, ended

    def serve_fsm(self, prompts, max_tokens, eos, top_k, temp, seed, fsm_start, rep=1.0, freq=0.0, pres=0.0, last_n=0, count_prompt=True, top_p=1.0,
                  min_p=0.0, tables=None, min_new=None, slice_steps=16, max_new=0, max_new_each=None, n_top=None):
        """serve_penalized() with a start state per prompt (a scalar for all; -1: not bound): (ids per prompt, stats, ended_by int32[prompts]);
        with n_top also serve_logprobs()'s records (log-probs, top ids, top log-probs) behind them"""
        n = len(prompts)
        args, rec = _records(n_top, n, max(max_tokens, max(len(p) for p in prompts)))
        if n_top is None:
            args = [None, 0, None, None, None]
        pen = _penalty_arg(n, rep, freq, pres, last_n, count_prompt)
        st, ended = np.ascontiguousarray(np.broadcast_to(np.asarray(fsm_start, np.int32), (n,))), np.zeros(n, np.int32)
        ids, stats = self._serve(self.host._bserve_fsm, "batch_serve_fsm", prompts, max_tokens, eos, slice_steps, max_new, max_new_each,
                                 *_request_args(n, top_k, temp, seed), *_full_args(n, (tables, np.int32), (min_new, np.int32)),
                                 *args, *_cut_args(n, top_p, min_p), C.byref(pen), _ptr(st), _ptr(ended))
        return (ids, stats, ended) if n_top is None else (ids, stats, ended, *rec)

    def generate_mirostat(self, prompts, max_tokens, tau, eta=0.1, eos=-1, top_k=40, temp=1.0, seed=0, streams=None, rep=1.0, freq=0.0, pres=0.0,
                          last_n=0, count_prompt=True, top_p=1.0, min_p=0.0, tables=None, min_new=None, fsm_start=-1):
        """generate_fsm() with a Mirostat request per sequence (tau / eta a scalar or a list; tau 0: off): the ids per sequence"""
        n = self.n_seq
        pen = _penalty_arg(n, rep, freq, pres, last_n, count_prompt)
        st, ended = np.ascontiguousarray(np.broadcast_to(np.asarray(fsm_start, np.int32), (n,))), np.zeros(n, np.int32)
        ta = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, np.float32), (n,)))
        et = np.ascontiguousarray(np.broadcast_to(np.asarray(eta, np.float32), (n,)))
        return self._generate(self.host._bgen_miro, "batch_generate_mirostat", prompts, max_tokens, eos,
                              _request_args(n, top_k, temp, seed) + _full_args(n, (streams, np.uint32), (tables, np.int32), (min_new, np.int32)),
                              [None, 0, None, None, None] + _cut_args(n, top_p, min_p) + [C.byref(pen), _ptr(st), _ptr(ended), _ptr(ta), _ptr(et),
                                                                                        C.c_float(0.0), C.c_float(0.1)])

    def serve_mirostat(self, prompts, max_tokens, eos, top_k, temp, seed, tau, eta=0.1, rep=1.0, freq=0.0, pres=0.0, last_n=0, count_prompt=True,
                       top_p=1.0, min_p=0.0, tables=None, min_new=None, fsm_start=-1, slice_steps=16, max_new=0, max_new_each=None):
        """serve_fsm() with a Mirostat request per prompt (tau / eta a scalar or a list; tau 0: off): (ids per prompt, stats)"""
        n = len(prompts)
        pen = _penalty_arg(n, rep, freq, pres, last_n, count_prompt)
        st, ended = np.ascontiguousarray(np.broadcast_to(np.asarray(fsm_start, np.int32), (n,))), np.zeros(n, np.int32)
        ta = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, np.float32), (n,)))
        et = np.ascontiguousarray(np.broadcast_to(np.asarray(eta, np.float32), (n,)))
        return self._serve(self.host._bserve_miro, "batch_serve_mirostat", prompts, max_tokens, eos, slice_steps, max_new, max_new_each,
                           *_request_args(n, top_k, temp, seed), *_full_args(n, (tables, np.int32), (min_new, np.int32)),
                           None, 0, None, None, None, *_cut_args(n, top_p, min_p), C.byref(pen), _ptr(st), _ptr(ended), _ptr(ta), _ptr(et),
                           C.c_float(0.0), C.c_float(0.1))

    def serve_regex(self, prompts, patterns, eos, vocab, max_tokens, top_k=0, temp=1.0, seed=0, **kw):
        """serve_fsm() with one pattern (or None: not bound) per prompt: a pool of the DISTINCT patterns over `vocab` (what Fsm.set_vocab
        takes) becomes the shared decoder's pool -- expanded on the device -- and every prompt starts in its pattern's start state.
        Returns serve_fsm()'s tuple with the list of start states behind it.  kw: serve_fsm's."""
        f = Fsm(self.host, self.cfg.n_vocab)
        try:
            f.set_vocab(vocab)
            starts = [-1 if p is None else f.add_regex(p, eos) for p in patterns]
            if f.n_states > 0:
                self.set_fsm(f)
            return (*self.serve_fsm(prompts, max_tokens, eos, top_k, temp, seed, starts, **kw), starts)
        finally:
            f.close()

    def serve_stop_text(self, prompts, strings_per_prompt, eos, vocab, max_tokens, top_k=0, temp=1.0, seed=0, **kw):
        """serve_fsm() with a list of stop strings (or None: not bound) per prompt: a pool of the DISTINCT lists as search ranges over `vocab`
        becomes the shared decoder's pool, expanded on the device.  Returns serve_fsm()'s tuple with, behind it, each prompt's new text
        (bytes) cut before its stop string.  kw: serve_fsm's."""
        f = Fsm(self.host, self.cfg.n_vocab)
        try:
            f.set_vocab(vocab)
            seen, starts = {}, []
            for strings in strings_per_prompt:
                key = tuple(_as_bytes(s) for s in strings) if strings else None
                if key is not None and key not in seen:
                    seen[key] = f.add_stop_text(strings)
                starts.append(-1 if key is None else seen[key])
            if f.n_states > 0:
                self.set_fsm(f)
            out = self.serve_fsm(prompts, max_tokens, eos, top_k, temp, seed, starts, **kw)
            texts = [_cut_text(self.host, f.vocab, ids[len(p):], s) for p, ids, s in zip(prompts, out[0], strings_per_prompt)]
            return (*out, texts)
        finally:
            f.close()

    def serve_json(self, prompts, schemas, eos, vocab, max_tokens, ws=0, depth=2, **kw):
        """serve_regex() with one schema (or None: not bound) per prompt, each as json_schema_regex(schema, ws, depth)"""
        patterns = [None if s is None else json_schema_regex(self.host, s, ws, depth) for s in schemas]
        return self.serve_regex(prompts, patterns, eos, vocab, max_tokens, **kw)

    # ---- sessions (include/gten_host_sessions.h)
    # ---- context shift (include/gten_host_shift.h)
    def _shift_ck(self, rc, what):
        if rc:
            raise GtenHipError(f"{what} rc={rc}: {self.host.shift_error() or self.host.hip._err().decode(errors='replace')}")

    def shift_rc(self, seqs, n_rows, keep, drop=0):
        seqs, n_rows = np.ascontiguousarray(seqs, dtype=np.int32), np.ascontiguousarray(n_rows, dtype=np.int32)
        assert len(seqs) == len(n_rows)
        return self.host._bshift(self.h, _ptr(seqs), _ptr(n_rows), int(keep), int(drop), len(seqs))

    def shift(self, seqs, n_rows, keep, drop=0):
        """gten_host_batch_shift: the caches of sequences seqs[i], n_rows[i] of their rows valid, shifted by (keep, drop) in one device call.
        Only the caches change: the ids and positions of the steps that follow are the caller's."""
        self._shift_ck(self.shift_rc(seqs, n_rows, keep, drop), "batch_shift")

    def kv_row_bytes(self):
        return self.host._bkv_row_bytes(self.h)

    def kv_read(self, seq, layer, row_from, rows):
        """(K, V) storage bytes of rows [row_from, row_from + rows) of sequence seq's caches on `layer`: uint8 [rows][row_bytes] each"""
        rb = self.kv_row_bytes()
        k, v = np.zeros((rows, rb), np.uint8), np.zeros((rows, rb), np.uint8)
        self._shift_ck(self.host._bkv_read(self.h, int(seq), int(layer), int(row_from), int(rows), _ptr(k), _ptr(v)), "batch_kv_read")
        return k, v

    def shift_info(self):
        """(sequence-shifts done, rows moved, rows dropped) through this batch"""
        u = [C.c_ulonglong(0) for _ in range(3)]
        self._ck(self.host._bshift_info(self.h, *[C.byref(x) for x in u]), "batch_shift_info")
        return tuple(x.value for x in u)

    def generate_shifting_rc(self, prompts, max_tokens, keep, drop=0, eos=-1, top_k=0, temp=1.0, seed=0, streams=None, rep=1.0, freq=0.0, pres=0.0,
                             last_n=0, count_prompt=True, top_p=1.0, min_p=0.0, table=-1, n_top=None):
        """gten_host_batch_generate_shifting: (rc, ids per sequence)"""
        assert len(prompts) == self.n_seq
        pr, npr, mp = _pack(prompts)
        out, tot = np.zeros((self.n_seq, max_tokens), np.int32), np.zeros(self.n_seq, np.int32)
        st = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
        pen = _penalty_arg(self.n_seq, rep, freq, pres, last_n, count_prompt)
        rc = self.host._bgen_shift(self.h, _ptr(pr), _ptr(npr), mp, max_tokens, eos, int(top_k), float(temp), C.c_uint64(int(seed)), _ptr(st), int(table),
                                   -1 if n_top is None else int(n_top), C.c_float(top_p), C.c_float(min_p), C.byref(pen), int(keep), int(drop), _ptr(out), _ptr(tot))
        return rc, [out[q, : tot[q]].copy() for q in range(self.n_seq)]

    def generate_shifting(self, prompts, max_tokens, keep, drop=0, **requests):
        """generate_penalized() of every sequence past the window (HostModel.generate_shifting): list of id arrays, prompt included"""
        rc, ids = self.generate_shifting_rc(prompts, max_tokens, keep, drop, **requests)
        self._shift_ck(rc, "batch_generate_shifting")
        return ids

    def session_shift_rc(self, s, keep, drop=0):
        return self.host._bsess_shift(self.h, int(s), int(keep), int(drop))

    def session_shift(self, s, keep, drop=0):
        """the session's set is shifted by (keep, drop) on the device; its ids become ids[:keep] + ids[keep + drop:], its rows rows - drop"""
        self._shift_ck(self.session_shift_rc(s, keep, drop), "batch_session_shift")

    def sessions_reserve(self, n):
        """room for n sessions in all (at most SESSIONS_MAX); each costs a cache set when it is first opened"""
        self._ck(self.host._bsess_reserve(self.h, int(n)), "batch_sessions_reserve")

    def session_open(self):
        """a new, empty session: its id (raises when every reserved one is open)"""
        s = self.host._bsess_open(self.h)
        if s < 0:
            raise GtenHipError("batch_session_open: no free session (sessions_reserve)")
        return s

    def session_close(self, s):
        self._ck(self.host._bsess_close(self.h, int(s)), "batch_session_close")

    def session_info(self, s):
        """(ids held, valid rows, prefix the set is marked with or -1, rows of that mark)"""
        a, b, c, d = (C.c_int(0) for _ in range(4))
        self._ck(self.host._bsess_info(self.h, int(s), C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "batch_session_info")
        return a.value, b.value, c.value, d.value

    def session_ids(self, s):
        n = self.host._bsess_ids(self.h, int(s), None, 0)
        if n < 0:
            raise GtenHipError("batch_session_ids rc=%d" % n)
        out = np.zeros(max(n, 1), np.int32)
        self.host._bsess_ids(self.h, int(s), _ptr(out), n)
        return out[:n].copy()

    def session_truncate_rc(self, s, n_ids):
        return self.host._bsess_truncate(self.h, int(s), int(n_ids))

    def session_truncate(self, s, n_ids):
        """the history is cut to n_ids ids (rows = min(rows, n_ids)); nothing moves on the device"""
        self._ck(self.session_truncate_rc(s, n_ids), "batch_session_truncate")

    def sessions_info(self):
        """(open sessions, K / V bytes per session, session items served, of them continued segments, rows computed, rows kept)"""
        a = C.c_int(0)
        u = [C.c_ulonglong(0) for _ in range(5)]
        self._ck(self.host._bsessions_info(self.h, C.byref(a), *[C.byref(x) for x in u]), "batch_sessions_info")
        return (a.value,) + tuple(x.value for x in u)

    def serve_sessions_rc(self, items, max_tokens, eos, top_k, temp, seed, fsm_start=-1, rep=1.0, freq=0.0, pres=0.0, last_n=0, count_prompt=True, top_p=1.0,
                          min_p=0.0, tables=None, min_new=None, slice_steps=16, max_new=0, max_new_each=None, stride=None):
        """gten_host_batch_serve_sessions: items = [(session or None, ids)] -- a plain prompt, or the NEW ids of a session's turn (may be
        empty).  Returns (rc, ids per item -- history included --, stats, ended_by).  stride: the width of the out rows (default: what
        holds max_tokens and every history + turn)."""
        n = len(items)
        sess = np.ascontiguousarray([-1 if s is None else int(s) for s, _ in items], dtype=np.int32)
        turns = [list(p) for _, p in items]
        if stride is None:
            stride = max([max_tokens] + [len(p) + (self.session_info(s)[0] if s is not None else 0) for s, p in items])
        mp = max([1] + [len(p) for p in turns])
        width = max(stride, mp) if stride > max_tokens else mp
        pr, npr = np.zeros((n, width), np.int32), np.zeros(n, np.int32)
        for j, p in enumerate(turns):
            pr[j, : len(p)] = p
            npr[j] = len(p)
        pen = _penalty_arg(n, rep, freq, pres, last_n, count_prompt)
        st, ended = np.ascontiguousarray(np.broadcast_to(np.asarray(fsm_start, np.int32), (n,))), np.zeros(n, np.int32)
        out, tot, stats = np.zeros((n, max(max_tokens, width)), np.int32), np.zeros(n, np.int32), np.zeros(len(SERVE_STATS), np.float64)
        each, _ = _each(max_new_each, n, np.int32)
        rc = self.host._bserve_sessions(self.h, _ptr(pr), _ptr(npr), n, width, max_tokens, eos, slice_steps, max_new, _ptr(each), _ptr(out), _ptr(tot),
                                        _ptr(stats), len(stats), *_request_args(n, top_k, temp, seed), *_full_args(n, (tables, np.int32), (min_new, np.int32)),
                                        None, 0, None, None, None, *_cut_args(n, top_p, min_p), C.byref(pen), _ptr(st), _ptr(ended), _ptr(sess))
        return rc, [out[j, : tot[j]].copy() for j in range(n)], dict(zip(SERVE_STATS, stats.tolist())), ended

    def serve_sessions(self, items, max_tokens, eos, top_k, temp, seed, **requests):
        """serve_fsm() with a session per item (serve_sessions_rc): (ids per item, stats, ended_by)"""
        rc, ids, stats, ended = self.serve_sessions_rc(items, max_tokens, eos, top_k, temp, seed, **requests)
        self._ck(rc, "batch_serve_sessions")
        return ids, stats, ended

    # ---- n samples per prompt (include/gten_host_samples.h)
    def serve_samples_items(self, prompts, n, max_tokens, eos, top_k, temp, seed, fsm_start=-1, rep=1.0, freq=0.0, pres=0.0, last_n=0, count_prompt=True,
                            top_p=1.0, min_p=0.0, tables=None, min_new=None, slice_steps=16, max_new=0, max_new_each=None, n_top=None):
        """gten_host_batch_serve_samples in the EXPANDED queue's order: prompt j is generated n[j] times (n: a scalar for all), sample i
        of prompt j is item sum(n[:j]) + i and draws with stream = its item number.  Every request -- top_k, temp, fsm_start, the
        penalties, the cut, tables, min_new, max_new_each, n_top -- is a scalar for everybody, one value per PROMPT (its samples
        share it) or one value per item.  Returns (ids per item, stats, ended_by int32[items]) and, with n_top, the items' records behind them."""
        ns = _samples_counts(n, len(prompts))
        items = int(ns.sum())

        def ex(v):                                                   # a per-prompt list becomes a per-item list; a per-item one stays
            if v is None or np.isscalar(v):
                return v
            assert len(v) in (len(prompts), items), "one value per prompt, or one per item of the expanded queue"
            return np.repeat(np.asarray(v), ns) if len(v) == len(prompts) else np.asarray(v)
        width = max(max_tokens, max(len(p) for p in prompts))
        nt = n_top if n_top is None or np.isscalar(n_top) else [-1 if v is None else v for v in n_top]
        args, rec = _records(ex(nt), items, width)
        if n_top is None:
            args = [None, 0, None, None, None]
        pen = _penalty_arg(items, ex(rep), ex(freq), ex(pres), ex(last_n), ex(count_prompt))
        st, ended = np.ascontiguousarray(np.broadcast_to(np.asarray(ex(fsm_start), np.int32), (items,))), np.zeros(items, np.int32)
        pr, npr, mp = _pack(prompts)
        out, tot, stats = np.zeros((items, width), np.int32), np.zeros(items, np.int32), np.zeros(len(SERVE_STATS), np.float64)
        each, _ = _each(ex(max_new_each), items, np.int32)
        self._ck(self.host._bserve_samples(self.h, _ptr(pr), _ptr(npr), len(prompts), mp, max_tokens, eos, slice_steps, max_new, _ptr(each), _ptr(out),
                                           _ptr(tot), _ptr(stats), len(stats), *_request_args(items, ex(top_k), ex(temp), seed),
                                           *_full_args(items, (ex(tables), np.int32), (ex(min_new), np.int32)), *args,
                                           *_cut_args(items, ex(top_p), ex(min_p)), C.byref(pen), _ptr(st), _ptr(ended), _ptr(ns), 0), "batch_serve_samples")
        ids = [out[e, : tot[e]].copy() for e in range(items)]
        stats = dict(zip(SERVE_STATS, stats.tolist()))
        return (ids, stats, ended) if n_top is None else (ids, stats, ended, *rec)

    def serve_samples(self, prompts, n, max_tokens, eos, top_k, temp, seed, n_top=None, best_of=None, **requests):
        """n samples per prompt: (samples, stats, ended_by) with samples[j] the list of prompt j's id arrays (prompt + new ids) and
        ended_by[j] their int32 reasons; with n_top also (log-probs, top ids, top log-probs), each a list of per-prompt arrays
        [samples][positions(, n_top)].  best_of=k keeps, per prompt, the first k samples in samples_rank's order (best first); if
        nobody asked for records it asks with n_top 0 itself and does not return them.  **requests: serve_samples_items' others."""
        ns = _samples_counts(n, len(prompts))
        asked = n_top is not None
        got = self.serve_samples_items(prompts, ns, max_tokens, eos, top_k, temp, seed, n_top=n_top if asked or best_of is None else 0, **requests)
        ids, stats, ended = got[:3]
        first = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        keep = []
        for j, p in enumerate(prompts):
            idx = np.arange(first[j], first[j + 1])
            if best_of is not None:
                order = self.host.samples_rank_records(got[3][idx], len(p), [len(ids[e]) - len(p) for e in idx])
                idx = idx[order[: int(best_of)]]
            keep.append(idx)
        res = ([[ids[e] for e in idx] for idx in keep], stats, [ended[idx].copy() for idx in keep])
        return res + tuple([r[idx].copy() for idx in keep] for r in got[3:]) if asked else res

    def samples_info(self):
        """(items that were copies of another item's prompt pass, prompt rows not computed for them, groups that read from a group
        record, marked groups that got none -- all counted since the batch was made --, group records in use now)"""
        a, b, c, d, e = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0), C.c_int(0)
        self._ck(self.host._bsamples_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)), "batch_samples_info")
        return a.value, b.value, c.value, d.value, e.value

    def group_decode_set_rc(self, g, seq, rows=0):
        """group record g of the shared decoder becomes a snapshot of rows [0, rows) of sequence seq's own caches (seq None: released):
        gten_hip_decoder_group_set's return code"""
        return self.host._bgdset(self.h, int(g), -1 if seq is None else int(seq), int(rows))

    def group_decode_share_rc(self, seq, g, rows):
        """gten_hip_decoder_group_share(seq, g, rows) on the shared decoder: 0, or the refusal's code"""
        return self.host._bgdshare(self.h, int(seq), int(g), int(rows))

    def groups_decode_info(self, seq, g=None):
        """the shared decoder's group records: (record sequence `seq` reads from or -1, leading chunks of 256 positions it reads there);
        with `g` also (rows of record g, imports of its copy so far, its sharers now)"""
        sg, ch, rows, imp, sh = C.c_int(-1), C.c_int(0), C.c_int(0), C.c_ulonglong(0), C.c_int(0)
        self._ck(self.host._bgdinfo(self.h, int(seq), 0 if g is None else int(g), C.byref(sg), C.byref(ch), C.byref(rows), C.byref(imp), C.byref(sh)),
                 "batch_groups_decode_info")
        return (sg.value, ch.value) if g is None else (sg.value, ch.value, rows.value, imp.value, sh.value)

    def set_groups_cap(self, cap):
        """group records a queue may hold at a time (0: never take one; up to GROUPS_MAX; -1: the default, which is 0 -- as measured)"""
        self._ck(self.host._bgroups_cap(self.h, int(cap)), "batch_set_groups_cap")

    def set_prefix_rc(self, tokens):
        """gten_host_batch_set_prefix's return code (0; -2: this batch does not process prompts as segments; < 0: bad arguments)"""
        tokens = np.ascontiguousarray([] if tokens is None else tokens, dtype=np.int32)
        return self.host._bsetprefix(self.h, tokens.ctypes.data_as(C.c_void_p) if len(tokens) else None, len(tokens))

    def set_prefix(self, tokens):
        """the ids later prompts may begin with (None / []: none), processed once: a prompt that begins with them and has at
        least 16 ids of its own is computed from there on, with the same logits, ids and cache rows (include/gten_host_prefix.h)"""
        self._ck(self.set_prefix_rc(tokens), "batch_set_prefix")

    def prefix_info(self):
        """(prefix length, prompts that took the short way so far, prompt rows computed so far in segmented calls)"""
        n, sh, rows = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._ck(self.host._bprefixinfo(self.h, C.byref(n), C.byref(sh), C.byref(rows)), "batch_prefix_info")
        return n.value, sh.value, rows.value

    def prefix_decode_info(self, seq=0):
        """the shared decoder's side of the prefix (include/gten_host_prefix_decode.h): (prefix length it holds, leading chunks of 256
        positions sequence `seq` reads from the ONE copy, imports of that copy so far, sequence imports that skipped shared chunks)"""
        n, ch, pi, sk = C.c_int(0), C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._ck(self.host._bpdinfo(self.h, seq, C.byref(n), C.byref(ch), C.byref(pi), C.byref(sk)), "batch_prefix_decode_info")
        return n.value, ch.value, pi.value, sk.value

    def prefix_decode_share_rc(self, seq, rows):
        """gten_hip_decoder_slot_share(seq, rows) on the shared decoder: 0, or the refusal's code"""
        return self.host._bpdshare(self.h, seq, rows)

    def set_prefix_at_rc(self, which, tokens):
        """gten_host_batch_prefixes_set's return code (0; -2: this batch does not process prompts as segments; -1: bad arguments)"""
        tokens = np.ascontiguousarray([] if tokens is None else tokens, dtype=np.int32)
        return self.host._bpsset(self.h, which, tokens.ctypes.data_as(C.c_void_p) if len(tokens) else None, len(tokens))

    def set_prefix_at(self, which, tokens):
        """set_prefix at index `which` of 8 (None / []: clear it): a later prompt takes the LONGEST registered prefix it begins with and
        has 16 ids behind; the other indices, and what decodes behind them, are left alone (include/gten_host_prefixes.h)"""
        self._ck(self.set_prefix_at_rc(which, tokens), "batch_prefixes_set")

    def prefixes_info(self, which):
        """(length of prefix `which`, prompts that took the short way behind it so far, rows computed for them)"""
        n, sh, rows = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._ck(self.host._bpsinfo(self.h, which, C.byref(n), C.byref(sh), C.byref(rows)), "batch_prefixes_info")
        return n.value, sh.value, rows.value

    def prefix_decode_info_at(self, seq, which=None):
        """the shared decoder's view of several prefixes: (prefix index sequence `seq` shares or -1, leading chunks of 256 positions it
        reads from that one copy); with `which` also (length of prefix `which` there, imports of its copy so far, its sharers now)"""
        w, ch, n, pi, sh = C.c_int(-1), C.c_int(0), C.c_int(0), C.c_ulonglong(0), C.c_int(0)
        self._ck(self.host._bpsdinfo(self.h, seq, C.byref(w), C.byref(ch), 0 if which is None else which, C.byref(n), C.byref(pi), C.byref(sh)),
                 "batch_prefixes_decode_info")
        return (w.value, ch.value) if which is None else (w.value, ch.value, n.value, pi.value, sh.value)

    def prefixes_decode_share_rc(self, seq, which, rows):
        """gten_hip_decoder_prefixes_share(seq, which, rows) on the shared decoder: 0, or the refusal's code"""
        return self.host._bpsdshare(self.h, seq, which, rows)

    def prefix_set_steps(self, which, tokens, n_first, steps):
        """tests: prefix `which`'s own single-sequence decoder rewrites rows n_first - 1 .. of the prefix's cache set; the
        registration at `which` ends (include/gten_host_prefixes.h, gten_host_batch_prefixes_steps)"""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        self._ck(self.host._bpssteps(self.h, which, tokens.ctypes.data_as(C.c_void_p), len(tokens), n_first, steps), "batch_prefixes_steps")

    def decode_result(self, seq, n):
        out = C.c_int32(-1)
        self._ck(self.host._bresult(self.h, seq, n, C.byref(out)), "batch_decode_result")
        return out.value

    def logits(self, seq):
        out = np.zeros(self.cfg.n_vocab, np.float32)
        self._ck(self.host._blogits(self.h, seq, out.ctypes.data_as(C.c_void_p)), "batch_logits")
        return out

    def seq_steps(self, seq, tokens, n_first, steps):
        """steps n_first .. n_first + steps - 1 of ONE sequence on its own single-sequence decoder (same caches as the shared one)"""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        self._ck(self.host._bseqsteps(self.h, seq, tokens.ctypes.data_as(C.c_void_p), len(tokens), n_first, steps), "batch_seq_steps")

    def kv_info(self):
        """(head-major K / V shadows kept, sequence imports launched so far, import launches) of the shared decoder"""
        hm, imp, lau = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._ck(self.host._bkvinfo(self.h, C.byref(hm), C.byref(imp), C.byref(lau)), "batch_kv_info")
        return bool(hm.value), imp.value, lau.value

    def time_family(self, family, n, reps=20):
        us, cnt = C.c_double(0.0), C.c_int(0)
        self._ck(self.host._btime(self.h, family, n, reps, C.byref(us), C.byref(cnt)), "batch_time_family")
        return us.value, cnt.value

    def close(self):
        if self.h:
            self.host._bfree(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_host = None


def load_host():
    global _host
    if _host is None:
        _host = GtenHost()
    return _host
