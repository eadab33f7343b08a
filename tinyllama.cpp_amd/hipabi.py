"""ctypes binding of include/gten_hip.h (libgten_hip.so).

This is plumbing for tests and bench.py: device buffers are plain HBM
allocations owned by the library, moved with explicit h2d/d2h copies.  There
is no CPU fallback: a missing library or a missing GPU raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

I32, F16, F32, Q8, Q4 = 0, 1, 2, 3, 4


class GtenHipError(RuntimeError):
    pass


def _sig(lib, name, res, args):
    f = getattr(lib, name)
    f.restype = res
    f.argtypes = args
    return f


class DeviceBuffer:
    """A byte range in HBM.  `.ptr` is the raw device address (int)."""

    def __init__(self, api, nbytes):
        self.api = api
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        api._check(api._malloc(C.byref(p), self.nbytes))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, api, arr):
        arr = np.ascontiguousarray(arr)
        buf = cls(api, arr.nbytes)
        buf.upload(arr)
        return buf

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        self.api._check(self.api._h2d(self.ptr + offset, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def download(self, dtype=np.uint8, shape=None, offset=0, nbytes=None):
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        out = np.empty(nbytes, dtype=np.uint8)
        self.api._check(self.api._d2h(out.ctypes.data_as(C.c_void_p), self.ptr + offset, nbytes))
        out = out.view(dtype)
        return out.reshape(shape) if shape is not None else out

    def zero(self, byte=0):
        self.api._check(self.api._memset(self.ptr, byte, self.nbytes))

    def view(self, offset):
        """the bytes from `offset` on as an operand: every operator method takes it where it takes a buffer"""
        return DeviceView(self, offset)

    def free(self):
        if self.ptr:
            self.api._check(self.api._free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceView:
    """An address inside a DeviceBuffer: `.ptr` is parent.ptr + offset.  Owns nothing; holds its parent so that the
    allocation outlives every view of it."""

    def __init__(self, parent, offset):
        offset = int(offset)
        if not 0 <= offset <= parent.nbytes:
            raise ValueError(f"view at {offset} of a buffer of {parent.nbytes} bytes")
        self.parent = parent
        self.offset = offset
        self.nbytes = parent.nbytes - offset

    @property
    def ptr(self):
        return self.parent.ptr + self.offset

    def view(self, offset):
        return DeviceView(self.parent, self.offset + int(offset))


class BlockDesc(C.Structure):
    """gten_hip_block_desc (include/gten_hip.h)"""
    _fields_ = ([(k, C.c_int) for k in ("adtype", "wdtype", "n_embd", "n_heads", "n_kv_heads", "n_ffn")] +
                [(k, C.c_void_p) for k in ("attn_norm_w", "wq", "wk", "wv", "wo", "ffn_norm_w", "wgate", "wup", "wdown", "inp",
                                           "attn_norm_out", "q", "k", "v", "attn_out", "o", "h", "ffn_norm_out", "gate", "up", "down", "out")])


class RowCtx(C.Structure):
    """gten_hip_row_ctx (include/gten_hip_continue.h)"""
    _fields_ = [("k", C.c_void_p), ("v", C.c_void_p), ("len", C.c_int32)]


class GtenHip:
    """Loaded libgten_hip.so with every symbol of include/gten_hip.h bound."""

    SYMBOLS = [
        "gten_hip_device_count", "gten_hip_init", "gten_hip_last_error", "gten_hip_stream", "gten_hip_sync", "gten_hip_select_stream", "gten_hip_stream_wait", "gten_hip_stream_idle",
        "gten_hip_malloc", "gten_hip_free", "gten_hip_memset", "gten_hip_memcpy_h2d", "gten_hip_memcpy_d2h",
        "gten_hip_memcpy_d2d", "gten_hip_prof_enable", "gten_hip_prof_read", "gten_hip_prof_family_name",
        "gten_hip_selftest_q8scale", "gten_hip_row_bytes", "gten_hip_pack_weight", "gten_hip_token_embed",
        "gten_hip_block_rows", "gten_hip_set_block_rows", "gten_hip_matmul_2d", "gten_hip_rms_norm", "gten_hip_rotary_emb", "gten_hip_silu", "gten_hip_mul",
        "gten_hip_add", "gten_hip_qkv_attn", "gten_hip_argmax_row", "gten_hip_set_prefill_exact", "gten_hip_set_decode_exact", "gten_hip_set_decode_persistent", "gten_hip_persist_status", "gten_hip_set_row_segments", "gten_hip_row_segments_ok", "gten_hip_copy_ranges",
        # fused single-token decoder: driven from C++ (host/tinyllama_model.h), listed here so that
        # the export check covers the whole header
        "gten_hip_decoder_create", "gten_hip_decoder_destroy", "gten_hip_decoder_set_tokens",
        "gten_hip_decoder_step", "gten_hip_decoder_steps", "gten_hip_decoder_generate", "gten_hip_decoder_generate_multi", "gten_hip_decoder_step_ragged", "gten_hip_decoder_result", "gten_hip_decoder_time_family",
        "gten_hip_decoder_create_multi", "gten_hip_decoder_set_tokens_seq", "gten_hip_decoder_result_seq",
        "gten_hip_decoder_logits_seq",
        "gten_hip_decoder_lane_info", "gten_hip_set_lane_skip", "gten_hip_decoder_slot_start", "gten_hip_decoder_slot_start_until", "gten_hip_decoder_slot_park", "gten_hip_decoder_slot_bind", "gten_hip_decoder_slots_apply", "gten_hip_decoder_run", "gten_hip_decoder_run_lanes", "gten_hip_decoder_slot_ids", "gten_hip_decoder_slot_ids_all",
        "gten_hip_set_kv_head_major", "gten_hip_decoder_kv_info", "gten_hip_kv_watch_selftest", "gten_hip_set_ffn_streamed", "gten_hip_set_wx_planes",
    ]
    # include/gten_hip_sample.h (top-k sampling on the device)
    SAMPLE_SYMBOLS = ["gten_hip_decoder_set_sampling", "gten_hip_sample_rows"]
    # include/gten_hip_bias.h (bias tables: constrained generation on the device)
    BIAS_SYMBOLS = ["gten_hip_decoder_set_bias_table", "gten_hip_decoder_set_seq_bias", "gten_hip_sample_rows_biased", "gten_hip_decoder_bias_info"]
    BIAS_TABLES = 16                                             # GTEN_HIP_BIAS_TABLES
    # include/gten_hip_logprobs.h (log-probs and top-N alternatives of the generated ids)
    LOGPROBS_SYMBOLS = ["gten_hip_decoder_set_logprobs", "gten_hip_decoder_logprobs", "gten_hip_decoder_logprobs_info", "gten_hip_row_top_logprobs"]
    LOGPROBS_TOP = 20                                            # GTEN_HIP_LOGPROBS_TOP
    # include/gten_hip_nucleus.h (top-p / min-p cuts of the draw)
    NUCLEUS_SYMBOLS = ["gten_hip_decoder_set_cut", "gten_hip_decoder_cut_info", "gten_hip_sample_rows_cut"]
    CUT_INFO = np.dtype([("Z", np.uint64), ("n_cand", np.int32), ("n_nucleus", np.int32), ("n_minp", np.int32), ("n_keep", np.int32)])   # gten_hip_cut_info
    # include/gten_hip_penalty.h (repetition / frequency / presence penalties on the ids a sequence already holds)
    PENALTY_SYMBOLS = ["gten_hip_decoder_set_penalty", "gten_hip_decoder_penalty_info", "gten_hip_penalize_rows", "gten_hip_sample_rows_pen"]
    PENALTY_HISTORY_MAX = 65535                                  # GTEN_HIP_PENALTY_HISTORY_MAX
    # include/gten_hip_fsm.h (token automata: stop sequences and masked grammars)
    FSM_SYMBOLS = ["gten_hip_fsm_check", "gten_hip_decoder_set_fsm", "gten_hip_decoder_set_seq_fsm", "gten_hip_decoder_fsm_info",
                   "gten_hip_decoder_slot_states", "gten_hip_mask_rows_fsm", "gten_hip_sample_rows_fsm"]
    # include/gten_hip_mirostat.h (Mirostat v2: integer surprise, mu per position)
    MIROSTAT_SYMBOLS = ["gten_hip_miro_lg16_host", "gten_hip_miro_update_host", "gten_hip_miro_q16_host", "gten_hip_decoder_set_seq_mirostat",
                        "gten_hip_decoder_mirostat_info", "gten_hip_decoder_slot_mus", "gten_hip_sample_rows_miro"]
    MIRO_INFO = np.dtype([("Z", np.uint64), ("Zk", np.uint64), ("q_id", np.uint64), ("n_cand", np.int32), ("n_keep", np.int32), ("s", np.int32),
                          ("mu_next", np.int32), ("pad", np.int32, (2,))])                          # gten_hip_miro_info
    MIRO_MU_MAX = 64 << 16                                       # GTEN_HIP_MIRO_MU_MAX
    MIRO_MU_DEFAULT = -(1 << 31)                                 # GTEN_HIP_MIRO_MU_DEFAULT: start at 2 * tau_q
    # include/gten_hip_regex.h (byte automata expanded over the vocabulary on the device)
    REGEX_SYMBOLS = ["gten_hip_fsm_expand", "gten_hip_fsm_check_dev", "gten_hip_decoder_set_vocab_bytes", "gten_hip_decoder_set_fsm_parts"]
    # include/gten_hip_stoptext.h (search automata -- stop strings given as text -- expanded over the vocabulary on the device)
    STOPTEXT_SYMBOLS = ["gten_hip_fsm_expand_search", "gten_hip_decoder_set_fsm_parts_ex"]
    FSM_EXPAND_CHUNK, FSM_EXPAND_PASS, FSM_EXPAND_STATES = 4096, 8, 64      # GTEN_HIP_FSM_EXPAND_*
    FSM_DEAD = 0xFFFF                                            # GTEN_HIP_FSM_DEAD
    FSM_MAX_BYTES = 1 << 30                                      # GTEN_HIP_FSM_MAX_BYTES
    AB_SYMBOLS = ["gten_hip_set_decode_attn_classic", "gten_hip_set_weight_resident_mb", "gten_hip_set_weight_resident_bytes", "gten_hip_weight_resident_bytes",
                  "gten_hip_decoder_resident", "gten_hip_decoder_resident_budget"]         # include/gten_hip_ab.h
    O_PLANES_SYMBOLS = ["gten_hip_set_decode_o_planes", "gten_hip_decode_o_planes", "gten_hip_decoder_o_planes"]    # include/gten_hip_oplanes.h
    SCORE_SYMBOLS = ["gten_hip_row_logprobs"]                    # include/gten_hip_score.h
    PREFIX_SYMBOLS = ["gten_hip_block_rows_prefixed"]            # include/gten_hip_prefix.h
    CONTINUE_SYMBOLS = ["gten_hip_block_rows_continued", "gten_hip_set_row_contexts"]       # include/gten_hip_continue.h
    PREFIX_DECODE_SYMBOLS = ["gten_hip_decoder_prefix_set", "gten_hip_decoder_slot_share", "gten_hip_decoder_prefix_info",
                             "gten_hip_set_prefix_decode_shared"]          # include/gten_hip_prefix_decode.h
    PREFIXES_SYMBOLS = ["gten_hip_decoder_prefixes_set", "gten_hip_decoder_prefixes_share",
                        "gten_hip_decoder_prefixes_info"]                  # include/gten_hip_prefixes.h
    GROUPS_SYMBOLS = ["gten_hip_decoder_group_set", "gten_hip_decoder_group_share",
                      "gten_hip_decoder_groups_info"]                      # include/gten_hip_groups.h
    # include/gten_hip_beam.h (beam search: the round, the in-place gather of the beams' K / V rows, their decoder form)
    BEAM_SYMBOLS = ["gten_hip_beam_round", "gten_hip_permute_sets", "gten_hip_decoder_beam_begin", "gten_hip_decoder_beam_round",
                    "gten_hip_decoder_beam_live", "gten_hip_decoder_beam_read", "gten_hip_decoder_beam_end", "gten_hip_decoder_beam_info"]
    BEAM_MAX = 8                                                 # GTEN_HIP_BEAM_MAX
    SHIFT_SYMBOLS = ["gten_hip_kv_shift"]                        # include/gten_hip_shift.h (context shift of K / V caches in place)
    SHIFT_ITEM = np.dtype([("k", np.uint64), ("v", np.uint64), ("n", np.int32), ("keep", np.int32), ("drop", np.int32), ("pad", np.int32)])
    EMBED_SYMBOLS = ["gten_hip_pool_rows"]                       # include/gten_hip_embed.h (rows of several texts pooled into one vector each)
    POOLINGS = {"mean": 0, "last": 1}                            # GTEN_HIP_POOL_*
    GROUPS_MAX = 64                                              # GTEN_GROUPS_MAX
    PREFIXES_MAX = 8                                             # GTEN_PREFIXES_MAX

    def __init__(self, path=None):
        path = path or _build.HIP_LIB
        if not os.path.exists(path):
            raise GtenHipError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        self.path = path
        self.lib = L = C.CDLL(path, mode=C.RTLD_GLOBAL)
        vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
        self._count = _sig(L, "gten_hip_device_count", ci, [])
        self._init = _sig(L, "gten_hip_init", ci, [ci])
        self._err = _sig(L, "gten_hip_last_error", C.c_char_p, [])
        self._stream = _sig(L, "gten_hip_stream", vp, [])
        self._sync = _sig(L, "gten_hip_sync", ci, [])
        self._selftest_q8 = _sig(L, "gten_hip_selftest_q8scale", ci, [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])
        self._malloc = _sig(L, "gten_hip_malloc", ci, [C.POINTER(vp), sz])
        self._free = _sig(L, "gten_hip_free", ci, [vp])
        self._memset = _sig(L, "gten_hip_memset", ci, [vp, ci, sz])
        self._h2d = _sig(L, "gten_hip_memcpy_h2d", ci, [vp, vp, sz])
        self._d2h = _sig(L, "gten_hip_memcpy_d2h", ci, [vp, vp, sz])
        self._d2d = _sig(L, "gten_hip_memcpy_d2d", ci, [vp, vp, sz])
        self._row_bytes = _sig(L, "gten_hip_row_bytes", sz, [ci, ci])
        self._prof_enable = _sig(L, "gten_hip_prof_enable", ci, [ci])
        self._prof_read = _sig(L, "gten_hip_prof_read", ci, [ci, C.POINTER(ci), C.POINTER(C.c_double)])
        self._prof_name = _sig(L, "gten_hip_prof_family_name", C.c_char_p, [ci])
        self._pack = _sig(L, "gten_hip_pack_weight", ci, [vp, ci, ci, ci, vp])
        self._embed = _sig(L, "gten_hip_token_embed", ci, [vp, ci, ci, vp, vp, ci, sz, ci, ci, ci])
        self._matmul = _sig(L, "gten_hip_matmul_2d", ci, [vp, ci, sz, vp, ci, vp, ci, sz, ci, ci, ci, ci])
        self._rms = _sig(L, "gten_hip_rms_norm", ci, [vp, ci, sz, vp, vp, sz, ci, ci, ci])
        self._rope = _sig(L, "gten_hip_rotary_emb", ci, [vp, ci, sz, ci, ci, ci, ci])
        self._silu = _sig(L, "gten_hip_silu", ci, [vp, vp, ci, sz, ci, ci, ci])
        self._mul = _sig(L, "gten_hip_mul", ci, [vp, vp, vp, ci, sz, ci, ci, ci])
        self._add = _sig(L, "gten_hip_add", ci, [vp, vp, vp, ci, sz, ci, ci, ci])
        self._attn = _sig(L, "gten_hip_qkv_attn", ci, [vp, vp, vp, vp, ci, sz, sz, sz, ci, ci, ci, ci, ci])
        self._prefill_exact = _sig(L, "gten_hip_set_prefill_exact", ci, [ci])
        self._block_rows = _sig(L, "gten_hip_block_rows", ci, [C.POINTER(BlockDesc), ci, ci])
        self._block_rows_prefixed = _sig(L, "gten_hip_block_rows_prefixed", ci, [C.POINTER(BlockDesc), ci, vp, vp, ci])
        self._set_row_contexts = _sig(L, "gten_hip_set_row_contexts", ci, [vp, ci, ci])
        self._block_rows_continued = _sig(L, "gten_hip_block_rows_continued", ci, [C.POINTER(BlockDesc), ci, ci])
        self._set_block_rows = _sig(L, "gten_hip_set_block_rows", ci, [ci])
        self._prefix_decode_shared = _sig(L, "gten_hip_set_prefix_decode_shared", ci, [ci])
        self._group_set = _sig(L, "gten_hip_decoder_group_set", ci, [vp, ci, vp, ci])
        self._group_share = _sig(L, "gten_hip_decoder_group_share", ci, [vp, ci, ci, ci])
        self._groups_info = _sig(L, "gten_hip_decoder_groups_info", ci, [vp, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci),
                                                                         C.POINTER(C.c_ulonglong), C.POINTER(ci)])
        self._decode_exact = _sig(L, "gten_hip_set_decode_exact", ci, [ci])
        self._decode_attn_classic = _sig(L, "gten_hip_set_decode_attn_classic", ci, [ci])
        self._decode_o_planes = _sig(L, "gten_hip_set_decode_o_planes", ci, [ci])
        self._decode_o_planes_get = _sig(L, "gten_hip_decode_o_planes", ci, [])
        self._decoder_o_planes = _sig(L, "gten_hip_decoder_o_planes", ci, [vp, C.POINTER(ci)])
        self._decode_persistent = _sig(L, "gten_hip_set_decode_persistent", ci, [ci])
        self._weight_resident_mb = _sig(L, "gten_hip_set_weight_resident_mb", ci, [ci])
        self._weight_resident_bytes = _sig(L, "gten_hip_set_weight_resident_bytes", ci, [C.c_longlong])
        self._weight_resident_get = _sig(L, "gten_hip_weight_resident_bytes", C.c_longlong, [])
        self._decoder_resident = _sig(L, "gten_hip_decoder_resident", ci, [vp, C.POINTER(ci), C.POINTER(C.c_longlong)])
        self._decoder_resident_budget = _sig(L, "gten_hip_decoder_resident_budget", ci, [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)])
        self._kv_head_major = _sig(L, "gten_hip_set_kv_head_major", ci, [ci])
        self._kv_watch_selftest = _sig(L, "gten_hip_kv_watch_selftest", ci, [])
        self._ffn_streamed = _sig(L, "gten_hip_set_ffn_streamed", ci, [ci])
        self._wx_planes = _sig(L, "gten_hip_set_wx_planes", ci, [ci])
        self._lane_skip = _sig(L, "gten_hip_set_lane_skip", ci, [ci])
        self._persist_status = _sig(L, "gten_hip_persist_status", ci, [C.POINTER(ci), C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), C.c_void_p, ci])
        self._set_row_segments = _sig(L, "gten_hip_set_row_segments", ci, [C.c_void_p, ci])
        self._copy_ranges = _sig(L, "gten_hip_copy_ranges", ci, [C.c_void_p, ci])
        self._set_sampling = _sig(L, "gten_hip_decoder_set_sampling", ci, [vp, ci, ci, C.c_float, C.c_uint64, C.c_uint32])
        self._sample_rows = _sig(L, "gten_hip_sample_rows", ci, [vp, ci, ci, C.c_longlong, vp, vp, C.c_uint64, vp, vp, vp])
        self._sample_rows_biased = _sig(L, "gten_hip_sample_rows_biased", ci, [vp, ci, ci, C.c_longlong, vp, C.c_longlong, vp, vp, C.c_uint64, vp, vp, vp])
        self._set_bias_table = _sig(L, "gten_hip_decoder_set_bias_table", ci, [vp, ci, vp, vp, ci, C.c_float])
        self._set_seq_bias = _sig(L, "gten_hip_decoder_set_seq_bias", ci, [vp, ci, ci, ci])
        self._bias_info = _sig(L, "gten_hip_decoder_bias_info", ci, [vp, C.POINTER(ci), vp, vp, ci, C.POINTER(vp)])
        self._set_logprobs = _sig(L, "gten_hip_decoder_set_logprobs", ci, [vp, ci, ci])
        self._dec_logprobs = _sig(L, "gten_hip_decoder_logprobs", ci, [vp, ci, ci, ci, ci, vp, vp, vp])
        self._logprobs_info = _sig(L, "gten_hip_decoder_logprobs_info", ci, [vp, C.POINTER(ci), vp, C.POINTER(vp), C.POINTER(C.c_longlong), C.POINTER(ci)])
        self._row_top_logprobs = _sig(L, "gten_hip_row_top_logprobs", ci, [vp, ci, ci, C.c_longlong, vp, ci, vp, vp, vp])
        self._set_cut = _sig(L, "gten_hip_decoder_set_cut", ci, [vp, ci, C.c_float, C.c_float])
        self._cut_info = _sig(L, "gten_hip_decoder_cut_info", ci, [vp, vp, vp, vp, C.POINTER(ci)])
        self._sample_rows_cut = _sig(L, "gten_hip_sample_rows_cut", ci, [vp, ci, ci, C.c_longlong, vp, C.c_longlong, vp, vp, C.c_uint64, vp, vp, vp, vp, vp, vp])
        self._set_penalty = _sig(L, "gten_hip_decoder_set_penalty", ci, [vp, ci, C.c_float, C.c_float, C.c_float, ci, ci])
        self._penalty_info = _sig(L, "gten_hip_decoder_penalty_info", ci, [vp, vp, vp, vp, vp, vp, C.POINTER(ci)])
        self._penalize_rows = _sig(L, "gten_hip_penalize_rows", ci, [vp, ci, ci, C.c_longlong, vp, C.c_longlong, vp, vp, vp, vp, vp, vp, C.c_longlong])
        self._sample_rows_pen = _sig(L, "gten_hip_sample_rows_pen", ci, [vp, ci, ci, C.c_longlong, vp, C.c_longlong, vp, vp, C.c_uint64, vp, vp, vp, vp,
                                                                         vp, vp, vp, vp, vp, vp, vp])
        self._fsm_check = _sig(L, "gten_hip_fsm_check", ci, [vp, vp, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong)])
        self._set_fsm = _sig(L, "gten_hip_decoder_set_fsm", ci, [vp, vp, vp, ci])
        self._set_seq_fsm = _sig(L, "gten_hip_decoder_set_seq_fsm", ci, [vp, ci, ci, ci])
        self._fsm_info = _sig(L, "gten_hip_decoder_fsm_info", ci, [vp, C.POINTER(ci), vp, vp, C.POINTER(ci), ci, ci, ci, vp, C.POINTER(vp), C.POINTER(vp)])
        self._slot_states = _sig(L, "gten_hip_decoder_slot_states", ci, [vp, ci, ci, ci, vp])
        self._slot_start_until = _sig(L, "gten_hip_decoder_slot_start_until", ci, [vp, ci, ci, ci])
        self._slot_park = _sig(L, "gten_hip_decoder_slot_park", ci, [vp, ci])
        self._decoder_run = _sig(L, "gten_hip_decoder_run", ci, [vp, ci])
        self._slot_ids = _sig(L, "gten_hip_decoder_slot_ids", ci, [vp, ci, ci, ci, vp])
        self._fsm_expand = _sig(L, "gten_hip_fsm_expand", ci, [vp, vp, ci, ci, ci, vp, C.c_longlong, vp, vp, vp, ci, ci])
        self._fsm_check_dev = _sig(L, "gten_hip_fsm_check_dev", ci, [vp, vp, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong)])
        self._set_vocab_bytes = _sig(L, "gten_hip_decoder_set_vocab_bytes", ci, [vp, vp, vp])
        self._fsm_expand_search = _sig(L, "gten_hip_fsm_expand_search", ci, [vp, vp, ci, ci, ci, vp, C.c_longlong, vp, vp, vp, ci])
        self._set_fsm_parts_ex = _sig(L, "gten_hip_decoder_set_fsm_parts_ex", ci, [vp, ci, vp, vp, ci])
        self._set_fsm_parts = _sig(L, "gten_hip_decoder_set_fsm_parts", ci, [vp, ci, vp, vp, ci])
        self._mask_rows_fsm = _sig(L, "gten_hip_mask_rows_fsm", ci, [vp, ci, ci, C.c_longlong, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, C.c_longlong])
        self._sample_rows_fsm = _sig(L, "gten_hip_sample_rows_fsm", ci, [vp, ci, ci, C.c_longlong, vp, vp, ci, vp, vp, vp, C.c_uint64, vp, vp, vp, vp,
                                                                         vp, vp, vp, vp, vp, vp, vp, vp])
        self._miro_lg16 = _sig(L, "gten_hip_miro_lg16_host", C.c_int32, [C.c_uint64])
        self._miro_update = _sig(L, "gten_hip_miro_update_host", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32])
        self._miro_q16 = _sig(L, "gten_hip_miro_q16_host", ci, [C.c_float, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_int32)])
        self._set_seq_mirostat = _sig(L, "gten_hip_decoder_set_seq_mirostat", ci, [vp, ci, C.c_float, C.c_float, C.c_int32, ci])
        self._mirostat_info = _sig(L, "gten_hip_decoder_mirostat_info", ci, [vp, vp, vp, vp, C.POINTER(ci), ci, ci, ci, vp])
        self._slot_mus = _sig(L, "gten_hip_decoder_slot_mus", ci, [vp, ci, ci, ci, vp])
        self._sample_rows_miro = _sig(L, "gten_hip_sample_rows_miro", ci, [vp, ci, ci, C.c_longlong, vp, C.c_longlong, vp, vp, ci, vp, vp, vp, C.c_uint64,
                                                                           vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])
        self._row_logprobs = _sig(L, "gten_hip_row_logprobs", ci, [vp, ci, ci, C.c_longlong, vp, vp, vp, vp])
        self._argmax_row = _sig(L, "gten_hip_argmax_row", ci, [vp, ci, vp])
        self._beam_round = _sig(L, "gten_hip_beam_round", ci, [vp, ci, vp, vp, vp, C.c_longlong, vp, ci, vp, vp, ci, vp])
        self._permute_sets = _sig(L, "gten_hip_permute_sets", ci, [vp, ci, sz, sz, vp, ci, vp, vp, ci])
        self._beam_begin = _sig(L, "gten_hip_decoder_beam_begin", ci, [vp, vp, ci, vp, ci])
        self._dec_beam_round = _sig(L, "gten_hip_decoder_beam_round", ci, [vp])
        self._beam_live = _sig(L, "gten_hip_decoder_beam_live", ci, [vp, C.POINTER(ci)])
        self._beam_read = _sig(L, "gten_hip_decoder_beam_read", ci, [vp, ci, vp, vp, vp])
        self._beam_end = _sig(L, "gten_hip_decoder_beam_end", ci, [vp])
        self._beam_info = _sig(L, "gten_hip_decoder_beam_info", ci, [vp, C.POINTER(ci), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)])
        self._kv_shift = _sig(L, "gten_hip_kv_shift", ci, [vp, ci, ci, sz, ci, ci])
        self._pool_rows = _sig(L, "gten_hip_pool_rows", ci, [vp, ci, sz, ci, vp, ci, ci, ci, vp])
        self.initialised = False

    # -- runtime
    def _check(self, rc):
        if rc != 0:
            raise GtenHipError(f"gten_hip error {rc}: {self._err().decode(errors='replace')}")

    def device_count(self):
        return self._count()

    def init(self, device=0):
        if self.device_count() <= device:
            raise GtenHipError(f"no MI355X visible (device_count={self.device_count()}, asked for {device}); "
                               "there is no CPU fallback for the gten_hip path")
        self._check(self._init(device))
        self.initialised = True
        return self

    def sync(self):
        self._check(self._sync())

    def selftest_q8scale(self):
        """(mismatches of div127, mismatches of recip_rn) against the IEEE division expansion, on the device"""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._selftest_q8(C.byref(a), C.byref(b)))
        return a.value, b.value

    def stream(self):
        return self._stream()

    def set_row_segments(self, starts):
        """rows [starts[k], starts[k + 1]) of the next gten_hip_block_rows calls are prompt k (None / []: one prompt)"""
        if not starts:
            self._check(self._set_row_segments(None, 0))
            return
        a = np.ascontiguousarray(starts, dtype=np.int32)
        self._check(self._set_row_segments(a.ctypes.data_as(C.c_void_p), len(a) - 1))

    def copy_ranges(self, ranges):
        """ranges: [(dst_ptr, src_ptr, nbytes)] device-to-device, one launch"""
        self._check(self.copy_ranges_rc(ranges))

    def copy_ranges_rc(self, ranges):
        """the return code of one gten_hip_copy_ranges call (a null address is passed as it is: the library refuses it)"""
        class R(C.Structure):
            _fields_ = [("dst", C.c_void_p), ("src", C.c_void_p), ("bytes", C.c_size_t)]
        arr = (R * max(len(ranges), 1))(*[R(int(d) or None, int(s) or None, int(b)) for d, s, b in ranges])
        return self._copy_ranges(C.cast(arr, C.c_void_p), len(ranges))

    def sample_rows(self, logits, n_rows, n_vocab, row_stride, top_k, temp, seed, stream, position):
        """ids of gten_hip_sample_rows (include/gten_hip_sample.h): `logits` a DeviceBuffer of f32 rows, row r at r * row_stride
        elements; top_k / temp / stream / position per row (scalars are broadcast).  Returns int32[n_rows]."""
        def per_row(v, dt):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n_rows,)))
            return a, a.ctypes.data_as(C.c_void_p)
        (k, kp), (t, tp), (s, sp), (p, pp) = (per_row(top_k, np.int32), per_row(temp, np.float32), per_row(stream, np.uint32),
                                              per_row(position, np.int32))
        out = DeviceBuffer(self, max(4 * n_rows, 4))
        self._check(self._sample_rows(logits.ptr, n_rows, n_vocab, row_stride, kp, tp, C.c_uint64(int(seed)), sp, pp, out.ptr))
        return out.download(np.int32)[:n_rows].copy()

    def sample_rows_rc(self, logits, n_rows, n_vocab, row_stride, top_k, temp, seed=0, stream=0, position=1):
        """the return code of one gten_hip_sample_rows call (argument checks); out is a scratch word"""
        k, t = np.full(max(n_rows, 1), top_k, np.int32), np.full(max(n_rows, 1), temp, np.float32)
        s, p = np.full(max(n_rows, 1), stream, np.uint32), np.full(max(n_rows, 1), position, np.int32)
        out = DeviceBuffer(self, 4 * max(n_rows, 1))
        return self._sample_rows(logits.ptr, n_rows, n_vocab, row_stride, k.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p),
                                 C.c_uint64(int(seed)), s.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), out.ptr)

    def sample_rows_biased(self, logits, bias, n_rows, n_vocab, row_stride, bias_stride, top_k, temp, seed, stream, position):
        """ids of gten_hip_sample_rows_biased (include/gten_hip_bias.h): sample_rows on logits + bias, `bias` a DeviceBuffer of f32
        rows, row r at r * bias_stride elements (0: one row for all).  Returns int32[n_rows]."""
        def per_row(v, dt):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n_rows,)))
            return a, a.ctypes.data_as(C.c_void_p)
        (k, kp), (t, tp), (s, sp), (p, pp) = (per_row(top_k, np.int32), per_row(temp, np.float32), per_row(stream, np.uint32),
                                              per_row(position, np.int32))
        out = DeviceBuffer(self, max(4 * n_rows, 4))
        self._check(self._sample_rows_biased(logits.ptr, n_rows, n_vocab, row_stride, bias.ptr, bias_stride, kp, tp, C.c_uint64(int(seed)), sp, pp,
                                             out.ptr))
        return out.download(np.int32)[:n_rows].copy()

    def sample_rows_cut(self, logits, n_rows, n_vocab, row_stride, top_k, temp, seed, stream, position, top_p, min_p, bias=None, bias_stride=0,
                        info=True):
        """gten_hip_sample_rows_cut (include/gten_hip_nucleus.h): sample_rows (sample_rows_biased when `bias` is given) with row r cut
        by (top_p[r], min_p[r]); scalars are broadcast.  Returns (ids int32[n_rows], info) -- info a structured array of dtype CUT_INFO
        (Z, n_cand, n_nucleus, n_minp, n_keep), or None with info=False."""
        def per_row(v, dt):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n_rows,)))
            return a, a.ctypes.data_as(C.c_void_p)
        (k, kp), (t, tp), (s, sp), (p, pp) = (per_row(top_k, np.int32), per_row(temp, np.float32), per_row(stream, np.uint32),
                                              per_row(position, np.int32))
        (tpv, tpp), (mpv, mpp) = per_row(top_p, np.float32), per_row(min_p, np.float32)
        out = DeviceBuffer(self, max(4 * n_rows, 4))
        inf = DeviceBuffer(self, max(self.CUT_INFO.itemsize * n_rows, 8)) if info else None
        self._check(self._sample_rows_cut(logits.ptr, n_rows, n_vocab, row_stride, bias.ptr if bias is not None else None, bias_stride, kp, tp,
                                          C.c_uint64(int(seed)), sp, pp, tpp, mpp, out.ptr, inf.ptr if info else None))
        ids = out.download(np.int32)[:n_rows].copy()
        return ids, (inf.download(np.uint8)[: self.CUT_INFO.itemsize * n_rows].view(self.CUT_INFO).copy() if info else None)

    def sample_rows_cut_rc(self, logits, n_rows, n_vocab, row_stride, top_k=40, temp=1.0, top_p=0.9, min_p=0.0):
        """the return code of one gten_hip_sample_rows_cut call (argument checks); out is a scratch word"""
        m = max(n_rows, 1)
        k, t = np.full(m, top_k, np.int32), np.full(m, temp, np.float32)
        s, p = np.zeros(m, np.uint32), np.ones(m, np.int32)
        a, b = np.full(m, top_p, np.float32), np.full(m, min_p, np.float32)
        out = DeviceBuffer(self, 4 * m)
        v = lambda z: z.ctypes.data_as(C.c_void_p)
        return self._sample_rows_cut(logits.ptr, n_rows, n_vocab, row_stride, None, 0, v(k), v(t), C.c_uint64(0), v(s), v(p), v(a), v(b), out.ptr, None)

    @staticmethod
    def _windows(hist, n_rows):
        """(ids int32[total], offsets int32[n_rows + 1]) of per-row windows: a list of n_rows id lists, or one list for every row"""
        if n_rows and (len(hist) == 0 or np.isscalar(hist[0])):
            hist = [hist] * n_rows
        assert len(hist) == n_rows
        off = np.zeros(n_rows + 1, np.int32)
        off[1:] = np.cumsum([len(h) for h in hist])
        ids = np.ascontiguousarray(np.concatenate([np.asarray(h, np.int32).reshape(-1) for h in hist]) if n_rows else [], dtype=np.int32)
        return ids, off

    def penalize_rows(self, logits, n_rows, n_vocab, row_stride, hist, r, freq, pres, bias=None, bias_stride=0):
        """gten_hip_penalize_rows (include/gten_hip_penalty.h): the rows the draw would be made from, f32[n_rows][n_vocab].  `hist`: row
        r's window of ids, a list per row (or one list for all); r / freq / pres per row (scalars are broadcast)."""
        def per_row(v, dt):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n_rows,)))
            return a, a.ctypes.data_as(C.c_void_p)
        (rr, rp), (ff, fp), (pp_, ppp) = per_row(r, np.float32), per_row(freq, np.float32), per_row(pres, np.float32)
        ids, off = self._windows(hist, n_rows)
        out = DeviceBuffer(self, max(4 * n_rows * n_vocab, 4))
        self._check(self._penalize_rows(logits.ptr, n_rows, n_vocab, row_stride, bias.ptr if bias is not None else None, bias_stride,
                                        ids.ctypes.data_as(C.c_void_p) if len(ids) else None, off.ctypes.data_as(C.c_void_p), rp, fp, ppp, out.ptr, n_vocab))
        return out.download(np.float32)[: n_rows * n_vocab].reshape(n_rows, n_vocab).copy()

    def sample_rows_pen(self, logits, n_rows, n_vocab, row_stride, top_k, temp, seed, stream, position, hist, r, freq, pres, top_p=1.0, min_p=0.0,
                        bias=None, bias_stride=0, info=False):
        """gten_hip_sample_rows_pen (include/gten_hip_penalty.h): sample_rows_cut with row r penalised by (r, freq, pres) over its window
        hist[r].  Returns (ids int32[n_rows], info or None) like sample_rows_cut."""
        def per_row(v, dt):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n_rows,)))
            return a, a.ctypes.data_as(C.c_void_p)
        (k, kp), (t, tp), (s, sp), (p, pp) = (per_row(top_k, np.int32), per_row(temp, np.float32), per_row(stream, np.uint32),
                                              per_row(position, np.int32))
        (a, tpp), (b, mpp) = per_row(top_p, np.float32), per_row(min_p, np.float32)
        (rr, rp), (ff, fp), (pr_, prp) = per_row(r, np.float32), per_row(freq, np.float32), per_row(pres, np.float32)
        ids, off = self._windows(hist, n_rows)
        out = DeviceBuffer(self, max(4 * n_rows, 4))
        inf = DeviceBuffer(self, max(self.CUT_INFO.itemsize * n_rows, 8)) if info else None
        self._check(self._sample_rows_pen(logits.ptr, n_rows, n_vocab, row_stride, bias.ptr if bias is not None else None, bias_stride, kp, tp,
                                          C.c_uint64(int(seed)), sp, pp, tpp, mpp, ids.ctypes.data_as(C.c_void_p) if len(ids) else None,
                                          off.ctypes.data_as(C.c_void_p), rp, fp, prp, out.ptr, inf.ptr if info else None))
        got = out.download(np.int32)[:n_rows].copy()
        return got, (inf.download(np.uint8)[: self.CUT_INFO.itemsize * n_rows].view(self.CUT_INFO).copy() if info else None)

    def sample_rows_pen_rc(self, logits, n_rows, n_vocab, row_stride, hist=(), r=1.1, freq=0.0, pres=0.0, top_k=40, temp=1.0):
        """the return code of one gten_hip_sample_rows_pen call (argument checks); out is a scratch word"""
        m = max(n_rows, 1)
        f = lambda v, dt: np.full(m, v, dt)                                                          # noqa: E731
        k, t, s, p, a, b = f(top_k, np.int32), f(temp, np.float32), f(0, np.uint32), f(1, np.int32), f(1.0, np.float32), f(0.0, np.float32)
        rr, ff, pp = f(r, np.float32), f(freq, np.float32), f(pres, np.float32)
        ids, off = self._windows(list(hist), m)
        out = DeviceBuffer(self, 4 * m)
        v = lambda z: z.ctypes.data_as(C.c_void_p)                                                  # noqa: E731
        return self._sample_rows_pen(logits.ptr, n_rows, n_vocab, row_stride, None, 0, v(k), v(t), C.c_uint64(0), v(s), v(p), v(a), v(b),
                                     v(ids) if len(ids) else None, v(off), v(rr), v(ff), v(pp), out.ptr, None)

    def decoder_set_penalty(self, dec, seq, r, freq, pres, start=0, last_n=0):
        """gten_hip_decoder_set_penalty on a raw decoder handle: sequence `seq` is penalised by (r, freq, pres) over the window
        (start, last_n) of its own ids; (1, 0, 0) clears it"""
        self._check(self._set_penalty(dec, int(seq), C.c_float(r), C.c_float(freq), C.c_float(pres), int(start), int(last_n)))

    def decoder_penalty_info(self, dec, n_seq):
        """gten_hip_decoder_penalty_info: (r f32[n_seq], freq, pres, start int32[n_seq], last_n, on)"""
        r, f, p = np.zeros(n_seq, np.float32), np.zeros(n_seq, np.float32), np.zeros(n_seq, np.float32)
        s, l = np.zeros(n_seq, np.int32), np.zeros(n_seq, np.int32)
        on = C.c_int(0)
        v = lambda z: z.ctypes.data_as(C.c_void_p)                                                  # noqa: E731
        self._check(self._penalty_info(dec, v(r), v(f), v(p), v(s), v(l), C.byref(on)))
        return r, f, p, s, l, bool(on.value)

    # ---- include/gten_hip_fsm.h
    def fsm_check(self, nxt, flags, n_vocab, n_states=None):
        """gten_hip_fsm_check on host tables (no device needed): (code, offending state or -1).  nxt: u16 [S][n_vocab], flags: u8 [S];
        n_states overrides S (the tables are then not looked at beyond what the early checks need)."""
        nxt = np.ascontiguousarray(nxt, dtype=np.uint16)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        where = C.c_longlong(-1)
        code = self._fsm_check(nxt.ctypes.data_as(C.c_void_p) if nxt.size else None, flags.ctypes.data_as(C.c_void_p) if flags.size else None,
                               int(len(flags) if n_states is None else n_states), int(n_vocab), C.byref(where))
        return code, int(where.value)

    def fsm_upload(self, nxt, flags):
        """a pool's tables as device buffers for the row operators: (next DeviceBuffer, flags DeviceBuffer, n_states)"""
        nxt = np.ascontiguousarray(nxt, dtype=np.uint16)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        dn, df = DeviceBuffer(self, max(nxt.nbytes, 4)), DeviceBuffer(self, max(flags.nbytes, 4))
        dn.upload(nxt)
        df.upload(flags)
        return dn, df, len(flags)

    # ---- include/gten_hip_regex.h
    def fsm_expand(self, pool, n_vocab, base, vocab, next256, accept, eos=-1):
        """gten_hip_fsm_expand into `pool` (fsm_upload()'s tuple: next, flags, n_states): rows [base, base + Sb (+ 1 with eos >= 0)) from the
        vocabulary `vocab` = (bytes u8[], offsets int32[n_vocab + 1]) and the byte automaton (next256 u16 [Sb][256], accept u8 [Sb]).
        Asynchronous on the library's stream; everything it reads is uploaded here and freed after a sync."""
        vb, vo = np.ascontiguousarray(vocab[0], dtype=np.uint8), np.ascontiguousarray(vocab[1], dtype=np.int32)
        n256, acc = np.ascontiguousarray(next256, dtype=np.uint16), np.ascontiguousarray(accept, dtype=np.uint8)
        assert n256.shape == (len(acc), 256) and len(vo) == n_vocab + 1
        pad = np.zeros(4, np.uint8)
        bufs = [self.upload(np.concatenate([vb, pad])), self.upload(vo), self.upload(n256), self.upload(acc)]
        try:
            self._check(self._fsm_expand(pool[0].ptr, pool[1].ptr, int(pool[2]), int(n_vocab), int(base), bufs[0].ptr, len(vb), bufs[1].ptr, bufs[2].ptr,
                                         bufs[3].ptr, len(acc), int(eos)))
            self.sync()
        finally:
            for b in bufs:
                b.free()

    def fsm_check_dev(self, pool, n_vocab, n_states=None):
        """gten_hip_fsm_check_dev on a device pool (fsm_upload()'s tuple): (code, offending state or -1), as fsm_check gives on the host"""
        where = C.c_longlong(-1)
        code = self._fsm_check_dev(pool[0].ptr, pool[1].ptr, int(pool[2] if n_states is None else n_states), int(n_vocab), C.byref(where))
        return code, int(where.value)

    def decoder_set_vocab_bytes(self, dec, vocab):
        """gten_hip_decoder_set_vocab_bytes: vocab = (bytes u8[], offsets int32[n_vocab + 1]); None drops it"""
        if vocab is None:
            return self._check(self._set_vocab_bytes(dec, None, None))
        vb, vo = np.ascontiguousarray(vocab[0], dtype=np.uint8), np.ascontiguousarray(vocab[1], dtype=np.int32)
        self._check(self._set_vocab_bytes(dec, vb.ctypes.data_as(C.c_void_p) if len(vb) else None, vo.ctypes.data_as(C.c_void_p)))

    class FsmPart(C.Structure):
        _fields_ = [("first", C.c_int), ("count", C.c_int), ("rows_host", C.c_void_p), ("next256_host", C.c_void_p), ("accept_host", C.c_void_p),
                    ("n_byte_states", C.c_int), ("eos", C.c_int)]

    def decoder_set_fsm_parts_rc(self, dec, n_states, flags, parts):
        """the return code of gten_hip_decoder_set_fsm_parts.  parts: in order, ("rows", u16 [count][n_vocab]) or
        ("regex", next256 u16 [Sb][256], accept u8 [Sb], eos); flags u8 [n_states] (read for the row parts)."""
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        keep, arr, at = [], (self.FsmPart * max(len(parts), 1))(), 0
        for k, p in enumerate(parts):
            if p[0] == "rows":
                rows = np.ascontiguousarray(p[1], dtype=np.uint16)
                keep.append(rows)
                arr[k] = self.FsmPart(at, len(rows), rows.ctypes.data, None, None, 0, -1)
                at += len(rows)
            else:
                n256, acc, eos = np.ascontiguousarray(p[1], dtype=np.uint16), np.ascontiguousarray(p[2], dtype=np.uint8), int(p[3])
                keep += [n256, acc]
                count = len(acc) + (1 if eos >= 0 else 0)
                arr[k] = self.FsmPart(at, count, None, n256.ctypes.data, acc.ctypes.data, len(acc), eos)
                at += count
        return self._set_fsm_parts(dec, int(n_states), flags.ctypes.data_as(C.c_void_p), C.cast(arr, C.c_void_p), len(parts))

    def decoder_set_fsm_parts(self, dec, n_states, flags, parts):
        self._check(self.decoder_set_fsm_parts_rc(dec, n_states, flags, parts))

    # ---- include/gten_hip_stoptext.h
    def fsm_expand_search(self, pool, n_vocab, base, vocab, next256, accept, n_bytes=None):
        """gten_hip_fsm_expand_search into `pool` (fsm_upload()'s tuple): rows [base, base + Sb] -- the last one the HIT state -- from the
        vocabulary `vocab` = (bytes u8[], offsets int32[n_vocab + 1]) and the search automaton (next256 u16 [Sb][256], accept u8 [Sb]).
        n_bytes: what the call is told the bytes' length is (None: len(bytes)).  Everything it reads is uploaded here and freed after a sync."""
        vb, vo = np.ascontiguousarray(vocab[0], dtype=np.uint8), np.ascontiguousarray(vocab[1], dtype=np.int32)
        n256, acc = np.ascontiguousarray(next256, dtype=np.uint16), np.ascontiguousarray(accept, dtype=np.uint8)
        assert n256.shape == (len(acc), 256) and len(vo) == n_vocab + 1
        assert n_bytes is None or 0 <= n_bytes <= len(vb)
        pad = np.zeros(4, np.uint8)
        bufs = [self.upload(np.concatenate([vb, pad])), self.upload(vo), self.upload(n256), self.upload(acc)]
        try:
            self._check(self._fsm_expand_search(pool[0].ptr, pool[1].ptr, int(pool[2]), int(n_vocab), int(base), bufs[0].ptr,
                                                len(vb) if n_bytes is None else int(n_bytes), bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, len(acc)))
            self.sync()
        finally:
            for b in bufs:
                b.free()

    class FsmPartEx(C.Structure):
        _fields_ = [("first", C.c_int), ("count", C.c_int), ("rows_host", C.c_void_p), ("next256_host", C.c_void_p), ("accept_host", C.c_void_p),
                    ("n_byte_states", C.c_int), ("eos", C.c_int), ("mode", C.c_int)]

    def decoder_set_fsm_parts_ex_rc(self, dec, n_states, flags, parts):
        """the return code of gten_hip_decoder_set_fsm_parts_ex.  parts: decoder_set_fsm_parts_rc's, or ("search", next256 u16 [Sb][256],
        accept u8 [Sb]): Sb + 1 states by the search rule."""
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        keep, arr, at = [], (self.FsmPartEx * max(len(parts), 1))(), 0
        for k, p in enumerate(parts):
            if p[0] == "rows":
                rows = np.ascontiguousarray(p[1], dtype=np.uint16)
                keep.append(rows)
                arr[k] = self.FsmPartEx(at, len(rows), rows.ctypes.data, None, None, 0, -1, 0)
                at += len(rows)
            else:
                n256, acc = np.ascontiguousarray(p[1], dtype=np.uint16), np.ascontiguousarray(p[2], dtype=np.uint8)
                search = p[0] == "search"
                eos = -1 if search else int(p[3])
                keep += [n256, acc]
                count = len(acc) + (1 if (search or eos >= 0) else 0)
                arr[k] = self.FsmPartEx(at, count, None, n256.ctypes.data, acc.ctypes.data, len(acc), eos, 1 if search else 0)
                at += count
        return self._set_fsm_parts_ex(dec, int(n_states), flags.ctypes.data_as(C.c_void_p), C.cast(arr, C.c_void_p), len(parts))

    def decoder_set_fsm_parts_ex(self, dec, n_states, flags, parts):
        self._check(self.decoder_set_fsm_parts_ex_rc(dec, n_states, flags, parts))

    def decoder_fsm_pool(self, dec, n_vocab):
        """the decoder's pool read back from the device through gten_hip_decoder_fsm_info's pointers: (next u16 [S][n_vocab], flags u8 [S])"""
        S, on, nd, fd = C.c_int(0), C.c_int(0), C.c_void_p(), C.c_void_p()
        self._check(self._fsm_info(dec, C.byref(S), None, None, C.byref(on), 0, 0, 0, None, C.byref(nd), C.byref(fd)))
        if S.value == 0:
            return np.zeros((0, n_vocab), np.uint16), np.zeros(0, np.uint8)
        nxt, flags = np.empty((S.value, n_vocab), np.uint16), np.empty(S.value, np.uint8)
        self.sync()
        self._check(self._d2h(nxt.ctypes.data_as(C.c_void_p), nd.value, nxt.nbytes))
        self._check(self._d2h(flags.ctypes.data_as(C.c_void_p), fd.value, flags.nbytes))
        return nxt, flags

    def mask_rows_fsm(self, logits, n_rows, n_vocab, row_stride, pool, states, hist=None, r=1.0, freq=0.0, pres=0.0):
        """gten_hip_mask_rows_fsm: the rows the draw would be made from, f32[n_rows][n_vocab].  pool: fsm_upload()'s tuple; states: one
        per row (-1: not bound); hist None: no penalties, otherwise as in penalize_rows."""
        def per_row(v, dt):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n_rows,)))
            return a, a.ctypes.data_as(C.c_void_p)
        (st, stp), (rr, rp), (ff, fp), (pp_, ppp) = per_row(states, np.int32), per_row(r, np.float32), per_row(freq, np.float32), per_row(pres, np.float32)
        ids, off = self._windows(hist, n_rows) if hist is not None else (np.zeros(0, np.int32), None)
        out = DeviceBuffer(self, max(4 * n_rows * n_vocab, 4))
        self._check(self._mask_rows_fsm(logits.ptr, n_rows, n_vocab, row_stride, pool[0].ptr, pool[1].ptr, pool[2], stp,
                                        ids.ctypes.data_as(C.c_void_p) if len(ids) else None, off.ctypes.data_as(C.c_void_p) if off is not None else None,
                                        rp, fp, ppp, out.ptr, n_vocab))
        return out.download(np.float32)[: n_rows * n_vocab].reshape(n_rows, n_vocab).copy()

    def sample_rows_fsm(self, logits, n_rows, n_vocab, row_stride, pool, states, top_k, temp, seed, stream, position, hist=None, r=1.0, freq=0.0,
                        pres=0.0, top_p=1.0, min_p=0.0, info=False):
        """gten_hip_sample_rows_fsm: sample_rows_pen (no bias) with row r in state states[r] of the pool.  Returns (ids int32[n_rows],
        next states int32[n_rows], info or None)."""
        def per_row(v, dt):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (n_rows,)))
            return a, a.ctypes.data_as(C.c_void_p)
        (k, kp), (t, tp), (s, sp), (p, pp) = (per_row(top_k, np.int32), per_row(temp, np.float32), per_row(stream, np.uint32),
                                              per_row(position, np.int32))
        (a, tpp), (b, mpp), (st, stp) = per_row(top_p, np.float32), per_row(min_p, np.float32), per_row(states, np.int32)
        (rr, rp), (ff, fp), (pr_, prp) = per_row(r, np.float32), per_row(freq, np.float32), per_row(pres, np.float32)
        ids, off = self._windows(hist, n_rows) if hist is not None else (np.zeros(0, np.int32), None)
        out, nxt = DeviceBuffer(self, max(4 * n_rows, 4)), DeviceBuffer(self, max(4 * n_rows, 4))
        inf = DeviceBuffer(self, max(self.CUT_INFO.itemsize * n_rows, 8)) if info else None
        self._check(self._sample_rows_fsm(logits.ptr, n_rows, n_vocab, row_stride, pool[0].ptr, pool[1].ptr, pool[2], stp, kp, tp, C.c_uint64(int(seed)),
                                          sp, pp, tpp, mpp, ids.ctypes.data_as(C.c_void_p) if len(ids) else None,
                                          off.ctypes.data_as(C.c_void_p) if off is not None else None, rp, fp, prp, out.ptr, nxt.ptr,
                                          inf.ptr if info else None))
        got, after = out.download(np.int32)[:n_rows].copy(), nxt.download(np.int32)[:n_rows].copy()
        return got, after, (inf.download(np.uint8)[: self.CUT_INFO.itemsize * n_rows].view(self.CUT_INFO).copy() if info else None)

    # -- Mirostat v2 (include/gten_hip_mirostat.h)
    def miro_lg16(self, x):
        """gten_hip_miro_lg16_host: lg16(x) in Q16; needs no device"""
        return int(self._miro_lg16(C.c_uint64(int(x))))

    def miro_update(self, mu, s, tau_q, eta_q):
        """gten_hip_miro_update_host: mu' of the contract's step 5; needs no device"""
        return int(self._miro_update(int(mu), int(s), int(tau_q), int(eta_q)))

    def miro_q16(self, tau, eta):
        """gten_hip_miro_q16_host: (code, tau_q, eta_q) -- code 0, or 1 / 2 for a tau / eta outside its range (tau_q, eta_q then None)"""
        a, b = C.c_int32(0), C.c_int32(0)
        rc = self._miro_q16(C.c_float(tau), C.c_float(eta), C.byref(a), C.byref(b))
        return (rc, a.value, b.value) if rc == 0 else (rc, None, None)

    def sample_rows_miro(self, logits, n_rows, n_vocab, row_stride, top_k, temp, seed, stream, position, mu, tau, eta, bias=None, bias_stride=0,
                         pool=None, states=-1, hist=None, r=1.0, freq=0.0, pres=0.0, info=True, rc=False):
        """gten_hip_sample_rows_miro: row r drawn under Mirostat (tau[r], eta[r]) with the threshold mu[r] (Q16); tau 0: the routine
        below.  pool: fsm_upload()'s tuple or None; hist None: no penalties; scalars are broadcast.  Returns (ids int32[n_rows], next
        states int32[n_rows], info of dtype MIRO_INFO or None); with rc=True the call's return code alone."""
        m = max(n_rows, 1)

        def per_row(v, dt):
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (m,)))
            return a, a.ctypes.data_as(C.c_void_p)
        (k, kp), (t, tp), (s, sp), (p, pp) = (per_row(top_k, np.int32), per_row(temp, np.float32), per_row(stream, np.uint32),
                                              per_row(position, np.int32))
        (muv, mup), (tav, tap), (etv, etp), (st, stp) = per_row(mu, np.int32), per_row(tau, np.float32), per_row(eta, np.float32), per_row(states, np.int32)
        (rr, rp), (ff, fp), (pr_, prp) = per_row(r, np.float32), per_row(freq, np.float32), per_row(pres, np.float32)
        ids, off = self._windows(hist, n_rows) if hist is not None else (np.zeros(0, np.int32), None)
        out, nxt = DeviceBuffer(self, 4 * m), DeviceBuffer(self, 4 * m)
        inf = DeviceBuffer(self, self.MIRO_INFO.itemsize * m) if info else None
        code = self._sample_rows_miro(logits.ptr, n_rows, n_vocab, row_stride, bias.ptr if bias is not None else None, bias_stride,
                                      pool[0].ptr if pool else None, pool[1].ptr if pool else None, pool[2] if pool else 0, stp if pool else None,
                                      kp, tp, C.c_uint64(int(seed)), sp, pp, ids.ctypes.data_as(C.c_void_p) if len(ids) else None,
                                      off.ctypes.data_as(C.c_void_p) if off is not None else None, rp, fp, prp, mup, tap, etp, out.ptr, nxt.ptr,
                                      inf.ptr if info else None)
        if rc:
            return code
        self._check(code)
        got, after = out.download(np.int32)[:n_rows].copy(), nxt.download(np.int32)[:n_rows].copy()
        return got, after, (inf.download(np.uint8)[: self.MIRO_INFO.itemsize * n_rows].view(self.MIRO_INFO).copy() if info else None)

    def decoder_set_seq_mirostat_rc(self, dec, seq, tau, eta=0.1, mu_q16=None, pos=0):
        return self._set_seq_mirostat(dec, int(seq), C.c_float(tau), C.c_float(eta), int(self.MIRO_MU_DEFAULT if mu_q16 is None else mu_q16), int(pos))

    def decoder_set_seq_mirostat(self, dec, seq, tau, eta=0.1, mu_q16=None, pos=0):
        """gten_hip_decoder_set_seq_mirostat: the ids of sequence seq from position pos on are drawn under Mirostat (tau, eta), mu starting
        at mu_q16 (None: 2 * tau_q); tau 0 unbinds"""
        self._check(self.decoder_set_seq_mirostat_rc(dec, seq, tau, eta, mu_q16, pos))

    def decoder_mirostat_info(self, dec, n_seq, row_seq=None, row_from=0, row_count=0):
        """gten_hip_decoder_mirostat_info: (tau_q int32[n_seq], eta_q int32[n_seq], pos int32[n_seq], on, mu row int32[row_count] or None)"""
        tq, eq, ps = np.zeros(n_seq, np.int32), np.zeros(n_seq, np.int32), np.zeros(n_seq, np.int32)
        on = C.c_int(0)
        row = np.zeros(max(row_count, 1), np.int32) if row_seq is not None else None
        v = lambda z: z.ctypes.data_as(C.c_void_p)                                                  # noqa: E731
        self._check(self._mirostat_info(dec, v(tq), v(eq), v(ps), C.byref(on), int(row_seq or 0), int(row_from), int(row_count),
                                        v(row) if row is not None else None))
        return tq, eq, ps, bool(on.value), (row[:row_count].copy() if row is not None else None)

    def decoder_slot_mus(self, dec, seq, n_from, count):
        """gten_hip_decoder_slot_mus: int32[count], entry i the mu (Q16) the id at position n_from + i is drawn under"""
        out = np.zeros(max(count, 1), np.int32)
        self._check(self._slot_mus(dec, int(seq), int(n_from), int(count), out.ctypes.data_as(C.c_void_p)))
        return out[:count].copy()

    def decoder_set_fsm_rc(self, dec, nxt, flags, n_states=None):
        """the return code of gten_hip_decoder_set_fsm (nxt None: the pool is dropped)"""
        if nxt is None:
            return self._set_fsm(dec, None, None, 0)
        nxt = np.ascontiguousarray(nxt, dtype=np.uint16)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        return self._set_fsm(dec, nxt.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p), int(len(flags) if n_states is None else n_states))

    def decoder_set_fsm(self, dec, nxt, flags):
        """gten_hip_decoder_set_fsm on a raw decoder handle: the decoder's automaton pool becomes (nxt u16 [S][n_vocab], flags u8 [S])"""
        self._check(self.decoder_set_fsm_rc(dec, nxt, flags))

    def decoder_set_seq_fsm_rc(self, dec, seq, state, pos=0):
        return self._set_seq_fsm(dec, int(seq), int(state), int(pos))

    def decoder_set_seq_fsm(self, dec, seq, state, pos=0):
        """gten_hip_decoder_set_seq_fsm: the id at position pos of sequence seq is chosen in `state`; -1 unbinds"""
        self._check(self._set_seq_fsm(dec, int(seq), int(state), int(pos)))

    def decoder_fsm_info(self, dec, n_seq, row_seq=None, row_from=0, row_count=0):
        """gten_hip_decoder_fsm_info: (n_states, state int32[n_seq], pos int32[n_seq], on, row int32[row_count] or None)"""
        st, ps = np.zeros(n_seq, np.int32), np.zeros(n_seq, np.int32)
        S, on = C.c_int(0), C.c_int(0)
        row = np.zeros(max(row_count, 1), np.int32) if row_seq is not None else None
        v = lambda z: z.ctypes.data_as(C.c_void_p)                                                  # noqa: E731
        self._check(self._fsm_info(dec, C.byref(S), v(st), v(ps), C.byref(on), int(row_seq or 0), int(row_from), int(row_count),
                                   v(row) if row is not None else None, None, None))
        return S.value, st, ps, bool(on.value), (row[:row_count].copy() if row is not None else None)

    def decoder_slot_states(self, dec, seq, n_from, count):
        """gten_hip_decoder_slot_states: int32[count], entry i the state the id at position n_from + i is chosen in"""
        out = np.zeros(max(count, 1), np.int32)
        self._check(self._slot_states(dec, int(seq), int(n_from), int(count), out.ctypes.data_as(C.c_void_p)))
        return out[:count].copy()

    def decoder_slot_start_until(self, dec, seq, n_first, n_last=0):
        """gten_hip_decoder_slot_start_until: slot seq runs free from step n_first and repeats step n_last once it is there (0: never)"""
        self._check(self._slot_start_until(dec, int(seq), int(n_first), int(n_last)))

    def decoder_slot_park(self, dec, seq):
        self._check(self._slot_park(dec, int(seq)))

    def decoder_run(self, dec, steps):
        """gten_hip_decoder_run: `steps` shared steps of every started slot, free-running"""
        self._check(self._decoder_run(dec, int(steps)))

    def decoder_slot_ids(self, dec, seq, n_from, count):
        """gten_hip_decoder_slot_ids: int32[count], the ids of steps [n_from, n_from + count) of slot seq"""
        out = np.zeros(max(count, 1), np.int32)
        self._check(self._slot_ids(dec, int(seq), int(n_from), int(count), out.ctypes.data_as(C.c_void_p)))
        return out[:count].copy()

    def decoder_set_cut(self, dec, seq, top_p, min_p):
        """gten_hip_decoder_set_cut on a raw decoder handle: sequence `seq` draws under (top_p, min_p); (1, 0) clears it"""
        self._check(self._set_cut(dec, int(seq), C.c_float(top_p), C.c_float(min_p)))

    def decoder_cut_info(self, dec, n_seq):
        """gten_hip_decoder_cut_info: (top_p f32[n_seq], min_p f32[n_seq], t f32[n_seq], on)"""
        a, b, t = np.zeros(n_seq, np.float32), np.zeros(n_seq, np.float32), np.zeros(n_seq, np.float32)
        on = C.c_int(0)
        self._check(self._cut_info(dec, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), C.byref(on)))
        return a, b, t, bool(on.value)

    def row_logprobs(self, logits, n_rows, n_vocab, row_stride, targets):
        """gten_hip_row_logprobs (include/gten_hip_score.h): `logits` a DeviceBuffer of f32 rows, row r at r * row_stride elements;
        targets int32[n_rows] (-1: not scored).  Returns (logprob f32[n_rows], rank int32[n_rows], argmax int32[n_rows])."""
        t = DeviceBuffer.from_numpy(self, np.ascontiguousarray(targets, dtype=np.int32))
        out = DeviceBuffer(self, 12 * n_rows)
        self._check(self._row_logprobs(logits.ptr, n_rows, n_vocab, row_stride, t.ptr, out.ptr, out.ptr + 4 * n_rows, out.ptr + 8 * n_rows))
        got = out.download(np.uint8)
        return got[: 4 * n_rows].view(np.float32).copy(), got[4 * n_rows: 8 * n_rows].view(np.int32).copy(), got[8 * n_rows:].view(np.int32).copy()

    def row_top_logprobs(self, logits, n_rows, n_vocab, row_stride, ids, n_top):
        """gten_hip_row_top_logprobs (include/gten_hip_logprobs.h): `logits` a DeviceBuffer of f32 rows, row r at r * row_stride elements;
        ids int32[n_rows] the chosen ids (-1: none, a scalar is broadcast).  Returns (logprob f32[n_rows], top_id int32[n_rows][n_top],
        top_logprob f32[n_rows][n_top]); entries from min(n_top, n_vocab) on are -1 / 0."""
        t = DeviceBuffer.from_numpy(self, np.ascontiguousarray(np.broadcast_to(np.asarray(ids, dtype=np.int32), (n_rows,))))
        w = max(n_top, 1)
        out = DeviceBuffer(self, 4 * n_rows * (1 + 2 * w))
        self._check(self._row_top_logprobs(logits.ptr, n_rows, n_vocab, row_stride, t.ptr, n_top, out.ptr, out.ptr + 4 * n_rows,
                                           out.ptr + 4 * n_rows * (1 + w)))
        self.sync()
        got = out.download(np.uint8)
        lp = got[: 4 * n_rows].view(np.float32).copy()
        ti = got[4 * n_rows: 4 * n_rows * (1 + w)].view(np.int32).reshape(n_rows, w)[:, :n_top].copy()
        tl = got[4 * n_rows * (1 + w):].view(np.float32).reshape(n_rows, w)[:, :n_top].copy()
        return lp, ti, tl

    def row_top_logprobs_rc(self, logits, n_rows, n_vocab, row_stride, n_top):
        """the return code of one gten_hip_row_top_logprobs call (argument checks); ids / outputs are scratch words"""
        buf = DeviceBuffer(self, 4 * max(n_rows, 1) * 48)
        buf.zero()
        r = 4 * max(n_rows, 1)
        return self._row_top_logprobs(logits.ptr, n_rows, n_vocab, row_stride, buf.ptr, n_top, buf.ptr + r, buf.ptr + 2 * r, buf.ptr + 24 * r)

    def row_logprobs_rc(self, logits, n_rows, n_vocab, row_stride):
        """the return code of one gten_hip_row_logprobs call (argument checks); targets / outputs are scratch words"""
        buf = DeviceBuffer(self, 16 * max(n_rows, 1))
        buf.zero()
        return self._row_logprobs(logits.ptr, n_rows, n_vocab, row_stride, buf.ptr, buf.ptr + 4 * max(n_rows, 1), None, None)

    def argmax_row(self, logits, n, offset=0):
        """gten_hip_argmax_row on the f32 row at byte `offset` of a DeviceBuffer: the greedy id (strict >, first maximum)"""
        out = DeviceBuffer(self, 4)
        self._check(self._argmax_row(logits.ptr + offset, n, out.ptr))
        return int(out.download(np.int32)[0])

    # -- beam search (include/gten_hip_beam.h).  BEAM_GROUP: one gten_hip_beam_group; BEAM_STATE: one gten_hip_beam_state (176 bytes)
    BEAM_GROUP = np.dtype([("row0", np.int32), ("n_beams", np.int32), ("prompt_len", np.int32), ("max_new", np.int32), ("eos", np.int32)])
    BEAM_STATE = np.dtype([("cum", np.float32, 8), ("fin_final", np.float32, 8), ("fin_cum", np.float32, 8), ("fin_t", np.int32, 8),
                           ("fin_beam", np.int32, 8), ("n_fin", np.int32), ("done", np.int32), ("t", np.int32), ("stepped", np.int32)])

    def beam_round(self, groups, state, top_id, top_lp, row_stride, w, n_w, parent, ids, trellis_rows, next_id):
        """gten_hip_beam_round on DeviceBuffers (groups: BEAM_GROUP records, state: BEAM_STATE records, in place); asynchronous"""
        self._check(self._beam_round(groups.ptr, groups.nbytes // self.BEAM_GROUP.itemsize, state.ptr, top_id.ptr, top_lp.ptr, int(row_stride), w.ptr,
                                     int(n_w), parent.ptr, ids.ptr, int(trellis_rows), next_id.ptr))

    def permute_sets_rc(self, ranges, offset, nbytes, groups, n_groups, state, parent, trellis_rows=1):
        """gten_hip_permute_sets: ranges = [(group, [base address of set 0, 1, ...])] (host), groups / state / parent device addresses
        (state 0 or None: parent is [n_groups][8]); the return code"""
        rec = np.zeros(len(ranges), np.dtype([("base", np.uint64, 8), ("group", np.int32), ("pad", np.int32)]))
        for i, (g, bases) in enumerate(ranges):
            rec["group"][i] = g
            rec["base"][i, : len(bases)] = bases
        return self._permute_sets(rec.ctypes.data_as(C.c_void_p), len(ranges), int(offset), int(nbytes), int(groups), int(n_groups),
                                  int(state) if state else None, int(parent), int(trellis_rows))

    def permute_sets(self, ranges, offset, nbytes, groups, n_groups, state, parent, trellis_rows=1):
        self._check(self.permute_sets_rc(ranges, offset, nbytes, groups, n_groups, state, parent, trellis_rows))

    # -- embeddings: rows pooled into one vector per segment (include/gten_hip_embed.h)
    def pool_rows_rc(self, dev, dtype, pitch, n_embd, starts, pooling="mean", normalize=True, out=None):
        """the return code of one gten_hip_pool_rows call (include/gten_hip_embed.h); `starts` holds the segment table, one more
        entry than there are segments.  out: a DeviceBuffer, by default a scratch with room for whatever an accepted call writes"""
        a = np.ascontiguousarray(starts, dtype=np.int32)
        if out is None:
            if getattr(self, "_pool_out", None) is None:
                self._pool_out = DeviceBuffer(self, 4 * 32 * 8192)
            out = self._pool_out
        code = self.POOLINGS.get(pooling, pooling)
        return self._pool_rows(dev.ptr if isinstance(dev, DeviceBuffer) else dev, int(dtype), int(pitch), int(n_embd), a.ctypes.data_as(C.c_void_p),
                               len(a) - 1, int(code), 1 if normalize else 0, out.ptr)

    def pool_rows(self, dev, dtype, pitch, n_embd, starts, pooling="mean", normalize=True):
        """gten_hip_pool_rows: segment k = rows [starts[k], starts[k + 1]) of the matrix at `dev` (a DeviceBuffer or a device address;
        dtype Q8 or F16, `pitch` bytes per row) pooled into one vector.  Returns f32 [len(starts) - 1][n_embd]."""
        T = len(starts) - 1
        out = DeviceBuffer(self, max(4 * T * n_embd, 64))
        self._check(self.pool_rows_rc(dev, dtype, pitch, n_embd, starts, pooling, normalize, out))
        return out.download(np.float32)[: T * n_embd].reshape(T, n_embd).copy()

    # -- context shift (include/gten_hip_shift.h)
    def kv_shift_rc(self, items, dtype, pitch, kv_dim, d_head):
        """the return code of one gten_hip_kv_shift call.  items: [(k_ptr, v_ptr, n, keep, drop)] -- device addresses (ints)"""
        a = np.zeros(len(items), self.SHIFT_ITEM)
        for i, (k, v, n, keep, drop) in enumerate(items):
            a[i] = (int(k), int(v), int(n), int(keep), int(drop), 0)
        return self._kv_shift(a.ctypes.data_as(C.c_void_p) if len(a) else None, len(a), int(dtype), int(pitch), int(kv_dim), int(d_head))

    def kv_shift(self, items, dtype, pitch, kv_dim, d_head):
        """gten_hip_kv_shift: every item's K / V rows [keep + drop, n) slide down to keep, K rotated back by drop; asynchronous"""
        self._check(self.kv_shift_rc(items, dtype, pitch, kv_dim, d_head))

    def decoder_beam_begin(self, dec, groups, w):
        """gten_hip_decoder_beam_begin on a raw decoder handle: groups = [(first_seq, n_beams, prompt_len, max_new, eos)], w the f32
        length weights; the return code (0, or a refusal: last_error())"""
        g = np.array([tuple(int(v) for v in x) for x in groups], dtype=self.BEAM_GROUP)
        w = np.ascontiguousarray(w, dtype=np.float32)
        return self._beam_begin(dec, g.ctypes.data_as(C.c_void_p), len(g), w.ctypes.data_as(C.c_void_p), len(w))

    def decoder_beam_round(self, dec):
        self._check(self._dec_beam_round(dec))

    def decoder_beam_live(self, dec):
        n = C.c_int(-1)
        self._check(self._beam_live(dec, C.byref(n)))
        return n.value

    def decoder_beam_read(self, dec, g, max_new):
        """(state as a BEAM_STATE record, parent int32[t][8], ids int32[t][8]) of group g"""
        st = np.zeros(1, self.BEAM_STATE)
        par, ids = np.zeros((max_new, 8), np.int32), np.zeros((max_new, 8), np.int32)
        self._check(self._beam_read(dec, int(g), st.ctypes.data_as(C.c_void_p), par.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)))
        t = int(st["t"][0])
        return st[0], par[:t].copy(), ids[:t].copy()

    def decoder_beam_end(self, dec):
        return self._beam_end(dec)

    def decoder_beam_info(self, dec):
        """(rounds since begin, bytes the last gather launch covered, gather launches so far)"""
        r, b, n = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._beam_info(dec, C.byref(r), C.byref(b), C.byref(n)))
        return r.value, b.value, n.value

    def last_error(self):
        return self._err().decode(errors="replace")

    def set_decode_exact(self, on):
        """exact forms of the decode step for decoders created from now on (include/gten_hip.h)"""
        self._check(self._decode_exact(1 if on else 0))

    def set_decode_attn_classic(self, on):
        """decoders created from now on: the single-sequence attention as k_dec_attn_one64w (0 / False, the default), as
        k_dec_attn_one64 (1 / True, the A/B control) or as k_dec_attn_one64v (2) -- the same bytes (include/gten_hip_ab.h)"""
        self._check(self._decode_attn_classic(int(on)))

    def set_decode_o_planes(self, on):
        """single-sequence decoders created from now on run their o launch as four K-quarter planes (1 / True, the default) or as
        one plane (0 / False, the A/B control) -- the same bytes (include/gten_hip_oplanes.h)"""
        self._check(self._decode_o_planes(int(on)))

    def decode_o_planes(self):
        """the setting a decoder created now would read: 1 or 0"""
        return int(self._decode_o_planes_get())

    def decoder_o_planes(self, dec):
        """what a raw decoder handle chose: 1 (k_dec_o_planes) or 0"""
        p = C.c_int(-1)
        self._check(self._decoder_o_planes(dec, C.byref(p)))
        return p.value

    def set_weight_resident_mb(self, mb):
        """single-sequence decoders created from now on keep the weights of their smallest W.x launches in the memory-side cache, up
        to `mb` MiB less their own K / V rows and scratch (0: every weight request nontemporal; include/gten_hip_ab.h)"""
        self._check(self._weight_resident_mb(int(mb)))

    def set_weight_resident_bytes(self, n):
        """set_weight_resident_mb to the byte"""
        self._check(self._weight_resident_bytes(int(n)))

    def weight_resident_bytes(self):
        """the setting a decoder created now would take, in bytes"""
        return int(self._weight_resident_get())

    def decoder_resident(self, dec):
        """(resident W.x launches, their weight bytes, the bytes the decoder had left for them, what it took off the setting first) of
        a raw decoder handle"""
        n, b, budget, over = C.c_int(0), C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        self._check(self._decoder_resident(dec, C.byref(n), C.byref(b)))
        self._check(self._decoder_resident_budget(dec, C.byref(budget), C.byref(over)))
        return n.value, b.value, budget.value, over.value

    def decoder_group_set(self, dec, g, kv, rows):
        """gten_hip_decoder_group_set on a raw decoder handle (include/gten_hip_groups.h): group record g becomes a snapshot of rows
        [0, rows) of the caches kv -- device addresses [n_layers][k, v] -- or is released (kv None); the return code"""
        if kv is None:
            return self._group_set(dec, int(g), None, 0)
        kv = np.ascontiguousarray(kv, dtype=np.uint64).reshape(-1, 2)
        return self._group_set(dec, int(g), kv.ctypes.data_as(C.c_void_p), int(rows))

    def decoder_group_share(self, dec, seq, g, rows):
        """gten_hip_decoder_group_share: "rows [0, rows) of sequence seq's own caches equal record g"; 0, or the refusal's code"""
        return self._group_share(dec, int(seq), int(g), int(rows))

    def decoder_groups_info(self, dec, seq, g=0):
        """gten_hip_decoder_groups_info: (record sequence seq reads from or -1, chunks it reads there, rows of record g, imports of
        record g's shadow so far, its sharers now)"""
        sg, ch, rows, imp, sh = C.c_int(-1), C.c_int(0), C.c_int(0), C.c_ulonglong(0), C.c_int(0)
        self._check(self._groups_info(dec, int(seq), int(g), C.byref(sg), C.byref(ch), C.byref(rows), C.byref(imp), C.byref(sh)))
        return sg.value, ch.value, rows.value, imp.value, sh.value

    def set_prefix_decode_shared(self, on):
        """decode slots behind a shared prefix read ONE copy of its K / V (default) or each its own (include/gten_hip_prefix_decode.h)"""
        self._check(self._prefix_decode_shared(-1 if on is None else 1 if on else 0))    # (None: the default again)

    def set_kv_head_major(self, on):
        """decoders of 16+ sequences created from now on: head-major shadows of the K / V caches (default) or the cache rows as they lie"""
        self._check(self._kv_head_major(1 if on else 0))

    def set_ffn_streamed(self, on):
        """gate | up of full 128-row q4 lanes as the streamed kernel (default) or as k_dec_mmvh: the same bits"""
        self._check(self._ffn_streamed(1 if on else 0))

    def set_wx_planes(self, on):
        """f16 wide decoders: o and down in eight K planes of 64-feature workgroups (default) or as k_dec_mmv_f16 in two"""
        self._check(self._wx_planes(1 if on else 0))

    def kv_watch_selftest(self):
        """host-only check of the watched-cache registry (no GPU needed): 0 = every case as expected, else the failing case"""
        return int(self._kv_watch_selftest())

    def set_decode_persistent(self, on):
        """single-sequence q4 decoders created from now on: the step as ONE persistent launch, or the launch chain (default)"""
        self._check(self._decode_persistent(1 if on else 0))

    def set_lane_skip(self, on):
        """1: gten_hip_decoder_run leaves lanes without a live slot out of the step; 0 (the library's default: skipping measured
        slower on the bench's queue): every run takes every lane"""
        self._check(self._lane_skip(1 if on else 0))

    def persist_status(self, n_stamps=0):
        """(decoders running the persistent step, launches enqueued, abort code [cleared], stamps) -- waits for the stream"""
        nd, nl, ab = C.c_int(0), C.c_ulonglong(0), C.c_uint(0)
        st = (C.c_uint * max(n_stamps, 1))()
        self._check(self._persist_status(C.byref(nd), C.byref(nl), C.byref(ab), C.cast(st, C.c_void_p) if n_stamps else None, n_stamps))
        return nd.value, nl.value, ab.value, list(st)[:n_stamps]

    def set_prefill_exact(self, on):
        """prompt-sized W.x with quantized weights: exact form (scalar-build order, bit for bit) instead of the fast one"""
        self._check(self._prefill_exact(1 if on else 0))

    def select_stream(self, idx):
        """queue the following calls on the library's stream 0 or 1 (include/gten_hip.h)"""
        self._check(self.lib.gten_hip_select_stream(int(idx)))

    def set_block_rows(self, on):
        """prompt-sized AttentionBlock calls as one composed call (default) or module by module"""
        self._check(self._set_block_rows(1 if on else 0))

    def block_rows(self, n, start_pos, ints, bufs):
        """gten_hip_block_rows: `ints` the six integers of the descriptor, `bufs` name -> DeviceBuffer.
        Returns False when the library does not take the configuration (GTEN_HIP_NOT_HANDLED)."""
        d = BlockDesc()
        for k, v in ints.items():
            setattr(d, k, int(v))
        for k, v in bufs.items():
            setattr(d, k, v.ptr)
        rc = self._block_rows(C.byref(d), n, start_pos)
        if rc == 1:
            return False
        self._check(rc)
        return True

    def block_rows_prefixed(self, n, ints, bufs, k_prefix, v_prefix, prefix_len):
        """gten_hip_block_rows_prefixed (include/gten_hip_prefix.h): block_rows for segments whose rows continue a shared prefix;
        k_prefix / v_prefix: DeviceBuffers (or device addresses) of the prefix's K / V rows of this layer"""
        d = BlockDesc()
        for k, v in ints.items():
            setattr(d, k, int(v))
        for k, v in bufs.items():
            setattr(d, k, v.ptr)
        rc = self._block_rows_prefixed(C.byref(d), n, getattr(k_prefix, "ptr", k_prefix), getattr(v_prefix, "ptr", v_prefix), int(prefix_len))
        if rc == 1:
            return False
        self._check(rc)
        return True

    def set_row_contexts(self, contexts):
        """gten_hip_set_row_contexts (include/gten_hip_continue.h): contexts[layer][s] = (k, v, len) of segment s of the row
        segments that are set -- k / v DeviceBuffers or device addresses of that segment's K / V rows [0, len) on the layer.
        None / []: clears."""
        if not contexts:
            self._check(self._set_row_contexts(None, 0, 0))
            return
        n_layers, n_seg = len(contexts), len(contexts[0])
        arr = (RowCtx * (n_layers * n_seg))()
        for l, row in enumerate(contexts):
            if len(row) != n_seg:
                raise ValueError("set_row_contexts: every layer lists the same segments")
            for s, (k, v, n) in enumerate(row):
                arr[l * n_seg + s] = RowCtx(getattr(k, "ptr", k), getattr(v, "ptr", v), int(n))
        self._check(self._set_row_contexts(C.cast(arr, C.c_void_p), n_layers, n_seg))

    def block_rows_continued(self, n, ints, bufs, layer=0):
        """gten_hip_block_rows_continued: block_rows for segments whose rows continue the contexts set for `layer`"""
        d = BlockDesc()
        for k, v in ints.items():
            setattr(d, k, int(v))
        for k, v in bufs.items():
            setattr(d, k, v.ptr)
        rc = self._block_rows_continued(C.byref(d), n, int(layer))
        if rc == 1:
            return False
        self._check(rc)
        return True

    def prof_enable(self, on):
        self._check(self._prof_enable(1 if on else 0))

    def prof_family_index(self, wanted):
        fam = 0
        while True:
            name = self._prof_name(fam)
            if name is None:
                raise KeyError(wanted)
            if name.decode() == wanted:
                return fam
            fam += 1

    def prof_read(self):
        """{family name: (launches, total_ms)} for every family with at least one launch."""
        out = {}
        fam = 0
        while True:
            name = self._prof_name(fam)
            if name is None:
                break
            n, ms = C.c_int(0), C.c_double(0.0)
            self._check(self._prof_read(fam, C.byref(n), C.byref(ms)))
            if n.value:
                out[name.decode()] = (n.value, ms.value)
            fam += 1
        return out

    def row_bytes(self, dtype, cols):
        return self._row_bytes(dtype, cols)

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def upload(self, arr):
        return DeviceBuffer.from_numpy(self, arr)

    def upload_weight(self, blocks, dtype, rows, cols):
        """uint8 [rows][row_bytes] in .gten block order -> packed device weight."""
        src = self.upload(blocks)
        dst = self.alloc(src.nbytes)
        self._check(self._pack(src.ptr, dtype, rows, cols, dst.ptr))
        self.sync()
        src.free()
        return dst

    # -- operators (DeviceBuffers or views of them; pitches default to dense rows).  The `_rc` forms return the code of the
    #    call instead of raising (0 = done; otherwise last_error() names the operator): what a refusal test reads
    def token_embed_rc(self, w, w_dtype, n_vocab, tokens, out, out_dtype, n, d, start_pos=0, out_pitch=None):
        return self._embed(w.ptr, w_dtype, n_vocab, tokens.ptr, out.ptr, out_dtype,
                           self.row_bytes(out_dtype, d) if out_pitch is None else out_pitch, n, d, start_pos)

    def token_embed(self, *a, **kw):
        self._check(self.token_embed_rc(*a, **kw))

    def matmul_2d_rc(self, x, x_dtype, w, w_dtype, out, out_dtype, n, d_in, d_out, start_pos=0,
                     x_pitch=None, out_pitch=None):
        return self._matmul(x.ptr, x_dtype, self.row_bytes(x_dtype, d_in) if x_pitch is None else x_pitch, w.ptr, w_dtype,
                            out.ptr, out_dtype, self.row_bytes(out_dtype, d_out) if out_pitch is None else out_pitch,
                            n, d_in, d_out, start_pos)

    def matmul_2d(self, *a, **kw):
        self._check(self.matmul_2d_rc(*a, **kw))

    def rms_norm_rc(self, x, dtype, w, out, n, d, start_pos=0, x_pitch=None, out_pitch=None):
        p = self.row_bytes(dtype, d)
        return self._rms(x.ptr, dtype, p if x_pitch is None else x_pitch, w.ptr, out.ptr, p if out_pitch is None else out_pitch,
                         n, d, start_pos)

    def rms_norm(self, *a, **kw):
        self._check(self.rms_norm_rc(*a, **kw))

    def rotary_emb_rc(self, x, dtype, n, d, d_head, start_pos=0, pitch=None):
        return self._rope(x.ptr, dtype, self.row_bytes(dtype, d) if pitch is None else pitch, n, d, d_head, start_pos)

    def rotary_emb(self, *a, **kw):
        self._check(self.rotary_emb_rc(*a, **kw))

    def silu_rc(self, x, out, dtype, n, d, start_pos=0, pitch=None):
        return self._silu(x.ptr, out.ptr, dtype, self.row_bytes(dtype, d) if pitch is None else pitch, n, d, start_pos)

    def silu(self, *a, **kw):
        self._check(self.silu_rc(*a, **kw))

    def mul_rc(self, a, b, out, dtype, n, d, start_pos=0, pitch=None):
        return self._mul(a.ptr, b.ptr, out.ptr, dtype, self.row_bytes(dtype, d) if pitch is None else pitch, n, d, start_pos)

    def mul(self, *a, **kw):
        self._check(self.mul_rc(*a, **kw))

    def add_rc(self, a, b, out, dtype, n, d, start_pos=0, pitch=None):
        return self._add(a.ptr, b.ptr, out.ptr, dtype, self.row_bytes(dtype, d) if pitch is None else pitch, n, d, start_pos)

    def add(self, *a, **kw):
        self._check(self.add_rc(*a, **kw))

    def qkv_attn_rc(self, q, k, v, out, dtype, n, n_heads, n_kv_heads, d_head, start_pos=0, q_pitch=None, kv_pitch=None,
                    out_pitch=None):
        qp = self.row_bytes(dtype, n_heads * d_head)
        kp = self.row_bytes(dtype, n_kv_heads * d_head)
        return self._attn(q.ptr, k.ptr, v.ptr, out.ptr, dtype, qp if q_pitch is None else q_pitch, kp if kv_pitch is None else kv_pitch,
                          qp if out_pitch is None else out_pitch, n, n_heads, n_kv_heads, d_head, start_pos)

    def qkv_attn(self, *a, **kw):
        self._check(self.qkv_attn_rc(*a, **kw))


_api = None


def load(device=None):
    """Process-wide GtenHip; initialised on `device` when given (needs a GPU)."""
    global _api
    if _api is None:
        _api = GtenHip()
    if device is not None and not _api.initialised:
        _api.init(device)
    return _api
