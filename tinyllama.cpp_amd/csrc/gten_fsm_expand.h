// gten_fsm_expand.h -- byte automata expanded over the vocabulary into the decoder's automaton pool, on the device
// (include/gten_hip_regex.h), and the check of a pool that lives there.  Included by gten_decode.hip behind its
// other entry points.  The definition the expansion is held to, byte for byte, is regex_expand() of host/regex_build.h.
//
// The expansion is a grid of independent short walks, one per (state, id), and one pass of stores over the rows it owns.  A workgroup
// takes FX_THREADS consecutive ids -- a thread one id -- and GTEN_HIP_FSM_EXPAND_STATES consecutive states.  The ids' bytes are one
// contiguous piece of the vocabulary: it is staged in LDS once (GTEN_HIP_FSM_EXPAND_CHUNK bytes at a time; a tile of longer pieces
// takes several rounds of the same loop, re-staged per pass) and walked by GTEN_HIP_FSM_EXPAND_PASS states at a time, whose current
// states a thread keeps in registers.  The automaton's 256-entry rows are read where they lie, through L2: nothing depends on how
// many states there are.  Every store instruction of a wave writes 64 consecutive u16 of one row, 128 contiguous bytes; the rows of
// a pass follow each other, so a workgroup leaves 512-byte runs per row behind.

#define FX_THREADS 256

// flags[base + s] of the automaton's states, and of the END state
__global__ __launch_bounds__(FX_THREADS) void k_fsm_expand_flags(uint8_t* __restrict__ flags, int base, const uint16_t* __restrict__ next256,
                                                                  const uint8_t* __restrict__ accept, int Sb, int eos)
{
    const int s = (int)blockIdx.x * FX_THREADS + (int)threadIdx.x;
    if (s < Sb) {
        const uint16_t* row = next256 + (size_t)s * 256;
        bool edge = false;
        for (int b = 0; b < 256; b++) edge |= (int)row[b] < Sb;
        flags[(size_t)base + (size_t)s] = (accept[s] && !edge) ? (uint8_t)GTEN_HIP_FSM_FINAL : (uint8_t)0;
    } else if (s == Sb && eos >= 0) {
        flags[(size_t)base + (size_t)Sb] = (uint8_t)GTEN_HIP_FSM_FINAL;
    }
}

__device__ __forceinline__ long long fx_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// rows [base, base + Sb + (eos >= 0)) of `next`; `flags` is what k_fsm_expand_flags left (the launch in front on the same stream)
__global__ __launch_bounds__(FX_THREADS) void k_fsm_expand(uint16_t* __restrict__ next, const uint8_t* __restrict__ flags, int V, int base,
                                                            const uint8_t* __restrict__ bytes, long long n_bytes, const int32_t* __restrict__ offsets,
                                                            const uint16_t* __restrict__ next256, const uint8_t* __restrict__ accept, int Sb, int eos)
{
    __shared__ uint8_t stage[GTEN_HIP_FSM_EXPAND_CHUNK];
    constexpr long long CH = GTEN_HIP_FSM_EXPAND_CHUNK;
    const int t0 = (int)blockIdx.x * FX_THREADS, t = t0 + (int)threadIdx.x;
    const int t1 = min(t0 + FX_THREADS, V);
    // the tile's bytes (uniform) and this thread's piece inside them; whatever the offsets hold, lo <= hi lie inside the tile
    const long long tile_lo = fx_clamp((long long)offsets[t0], 0, n_bytes), tile_hi = fx_clamp((long long)offsets[t1], tile_lo, n_bytes);
    long long lo = tile_lo, hi = tile_lo;
    if (t < V) {
        lo = fx_clamp((long long)offsets[t], tile_lo, tile_hi);
        hi = fx_clamp((long long)offsets[t + 1], lo, tile_hi);
    }
    const int n_rows = Sb + (eos >= 0 ? 1 : 0);
    const int s_begin = (int)blockIdx.y * GTEN_HIP_FSM_EXPAND_STATES, s_end = min(s_begin + GTEN_HIP_FSM_EXPAND_STATES, n_rows);
    const bool single = tile_hi - tile_lo <= CH;
    auto stage_from = [&](long long c0) {
        const long long cnt = min(CH, tile_hi - c0);
        for (long long j = threadIdx.x; j < cnt; j += FX_THREADS) stage[j] = bytes[c0 + j];
    };
    if (single) {
        stage_from(tile_lo);
        __syncthreads();
    }
    for (int s0 = s_begin; s0 < s_end; s0 += GTEN_HIP_FSM_EXPAND_PASS) {
        int cur[GTEN_HIP_FSM_EXPAND_PASS];
#pragma unroll
        for (int k = 0; k < GTEN_HIP_FSM_EXPAND_PASS; k++) cur[k] = (s0 + k < Sb && hi > lo) ? s0 + k : -1;       // (an empty piece, the END row: dead)
        for (long long c0 = tile_lo; c0 < tile_hi; c0 += CH) {
            if (!single) {
                __syncthreads();
                stage_from(c0);
                __syncthreads();
            }
            const long long a = max(lo, c0), b = min(hi, c0 + CH);
            for (long long j = a; j < b; j++) {
                const unsigned byte = stage[j - c0];
#pragma unroll
                for (int k = 0; k < GTEN_HIP_FSM_EXPAND_PASS; k++)
                    if (cur[k] >= 0) {
                        const int e = (int)next256[(size_t)cur[k] * 256 + byte];
                        cur[k] = e < Sb ? e : -1;
                    }
            }
        }
        if (t < V) {
#pragma unroll
            for (int k = 0; k < GTEN_HIP_FSM_EXPAND_PASS; k++) {
                const int s = s0 + k;
                if (s >= s_end) break;
                uint16_t v = cur[k] < 0 ? (uint16_t)GTEN_HIP_FSM_DEAD : (uint16_t)(base + cur[k]);
                if (t == eos)
                    v = (s < Sb && accept[s] && !(flags[(size_t)base + (size_t)s] & GTEN_HIP_FSM_FINAL)) ? (uint16_t)(base + Sb) : (uint16_t)GTEN_HIP_FSM_DEAD;
                next[((size_t)base + (size_t)s) * (size_t)V + (size_t)t] = v;
            }
        }
    }
}

// gten_hip_fsm_check's verdict on state blockIdx.x, folded into *result as min(2 * state + (stuck ? 1 : 0))
__global__ __launch_bounds__(FX_THREADS) void k_fsm_check(const uint16_t* __restrict__ next, const uint8_t* __restrict__ flags, int S, int V,
                                                           unsigned* __restrict__ result)
{
    __shared__ int bad_any[2];
    const int s = (int)blockIdx.x;
    if (threadIdx.x == 0) bad_any[0] = bad_any[1] = 0;
    __syncthreads();
    const uint16_t* row = next + (size_t)s * (size_t)V;
    bool bad = false, any = false;
    for (int i = (int)threadIdx.x; i < V; i += FX_THREADS) {
        const int e = (int)row[i];
        if (e == GTEN_HIP_FSM_DEAD) continue;
        if (e >= S) bad = true;
        else any = true;
    }
    if (bad) atomicOr(&bad_any[0], 1);
    if (any) atomicOr(&bad_any[1], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (bad_any[0]) atomicMin(result, 2u * (unsigned)s);
        else if (!bad_any[1] && !(flags[s] & GTEN_HIP_FSM_FINAL)) atomicMin(result, 2u * (unsigned)s + 1u);
    }
}

namespace {

// device allocations of a call that may leave early: freed at its end unless released to a new owner
struct FxScratch {
    std::vector<void*> ptrs;
    ~FxScratch() { for (void* p : ptrs) if (p) (void)hipFree(p); }
    hipError_t take(void** out, size_t bytes)
    {
        const hipError_t e = hipMalloc(out, bytes);
        if (e == hipSuccess) ptrs.push_back(*out);
        return e;
    }
    void release(void* p) { for (void*& q : ptrs) if (q == p) q = nullptr; }
};

int fx_launch(uint16_t* next_dev, uint8_t* flags_dev, int n_vocab, int base, const uint8_t* bytes, long long n_bytes, const int32_t* offsets,
              const uint16_t* next256, const uint8_t* accept, int Sb, int eos)
{
    const int n_rows = Sb + (eos >= 0 ? 1 : 0);
    GTR_LAUNCH(KT_DEC_SAMPLE, k_fsm_expand_flags, dim3((unsigned)((n_rows + FX_THREADS - 1) / FX_THREADS)), dim3(FX_THREADS), 0, flags_dev, base, next256, accept,
               Sb, eos);
    const dim3 grid((unsigned)((n_vocab + FX_THREADS - 1) / FX_THREADS), (unsigned)((n_rows + GTEN_HIP_FSM_EXPAND_STATES - 1) / GTEN_HIP_FSM_EXPAND_STATES));
    GTR_LAUNCH(KT_DEC_SAMPLE, k_fsm_expand, grid, dim3(FX_THREADS), 0, next_dev, (const uint8_t*)flags_dev, n_vocab, base, bytes, n_bytes, offsets, next256, accept,
               Sb, eos);
    return 0;
}

// the verdict of k_fsm_check over the whole pool: a code of gten_hip_fsm_check and *where
int fx_check(const uint16_t* next_dev, const uint8_t* flags_dev, int n_states, int n_vocab, int* code, long long* where)
{
    FxScratch tmp;
    unsigned* result = nullptr;
    GTR_CHECK(tmp.take((void**)&result, sizeof(unsigned)));
    GTR_CHECK(hipMemsetAsync(result, 0xFF, sizeof(unsigned), stream()));
    GTR_LAUNCH(KT_DEC_SAMPLE, k_fsm_check, dim3((unsigned)n_states), dim3(FX_THREADS), 0, next_dev, flags_dev, n_states, n_vocab, result);
    unsigned got = 0;
    GTR_CHECK(hipMemcpyAsync(&got, result, sizeof(got), hipMemcpyDeviceToHost, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    *code = got == 0xFFFFFFFFu ? GTEN_HIP_FSM_OK : ((got & 1u) ? GTEN_HIP_FSM_STUCK : GTEN_HIP_FSM_BAD_ENTRY);
    *where = got == 0xFFFFFFFFu ? -1 : (long long)(got >> 1);
    return 0;
}

} // namespace

extern "C" {

int gten_hip_fsm_expand(uint16_t* next_dev, uint8_t* flags_dev, int n_states, int n_vocab, int base, const uint8_t* bytes, long long n_bytes,
                        const int32_t* offsets, const uint16_t* next256, const uint8_t* accept, int n_byte_states, int eos)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(next_dev && flags_dev && offsets && next256 && accept && (bytes || n_bytes == 0), "fsm_expand: null argument");
    GTR_REQUIRE(n_states >= 1 && n_states <= GTEN_HIP_FSM_MAX_STATES && n_vocab >= 1 && n_vocab <= 65535, "fsm_expand: a pool of %d states over %d ids", n_states,
                n_vocab);
    GTR_REQUIRE(n_bytes >= 0 && n_bytes <= 0x7FFFFFFFll, "fsm_expand: %lld vocabulary bytes", n_bytes);
    GTR_REQUIRE(eos >= -1 && eos < n_vocab, "fsm_expand: eos %d outside [-1, %d)", eos, n_vocab);
    GTR_REQUIRE(n_byte_states >= 1 && base >= 0 && (long long)base + n_byte_states + (eos >= 0 ? 1 : 0) <= n_states,
                "fsm_expand: %d byte states (and the END state: %d) from state %d do not fit the pool's %d", n_byte_states, eos >= 0 ? 1 : 0, base, n_states);
    return fx_launch(next_dev, flags_dev, n_vocab, base, bytes, n_bytes, offsets, next256, accept, n_byte_states, eos);
}

int gten_hip_fsm_check_dev(const uint16_t* next_dev, const uint8_t* flags_dev, long long n_states, long long n_vocab, long long* where)
{
    if (where) *where = -1;
    if (!next_dev || !flags_dev || n_states < 1 || n_states > GTEN_HIP_FSM_MAX_STATES || n_vocab < 1 || n_vocab > 0x7FFFFFFFll) return GTEN_HIP_FSM_BAD_STATES;
    if ((unsigned long long)n_states * (unsigned long long)n_vocab * 2ull > GTEN_HIP_FSM_MAX_BYTES) return GTEN_HIP_FSM_TOO_LARGE;
    if (!gtr::inited()) return gtr::fail(-1, "gten_hip_init() has not been called");
    int code = 0;
    long long at = -1;
    if (const int rc = fx_check(next_dev, flags_dev, (int)n_states, (int)n_vocab, &code, &at)) return rc;
    if (where) *where = at;
    return code;
}

int gten_hip_decoder_set_vocab_bytes(gten_hip_decoder* dc, const uint8_t* bytes_host, const int32_t* offsets_host)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_set_vocab_bytes: null decoder");
    SamplerState& s = dc->smp;
    const int V = dc->d.n_vocab;
    FxScratch tmp;
    uint8_t* bytes = nullptr;
    int32_t* offsets = nullptr;
    long long n_bytes = 0;
    if (bytes_host || offsets_host) {
        GTR_REQUIRE(offsets_host && offsets_host[0] == 0, "decoder_set_vocab_bytes: offsets must start at 0");
        for (int i = 0; i < V; i++)
            GTR_REQUIRE(offsets_host[i + 1] >= offsets_host[i], "decoder_set_vocab_bytes: the offsets of id %d run backwards", i);
        n_bytes = offsets_host[V];
        GTR_REQUIRE(bytes_host || n_bytes == 0, "decoder_set_vocab_bytes: null bytes");
        GTR_CHECK(tmp.take((void**)&bytes, (size_t)std::max<long long>(n_bytes, 4)));
        GTR_CHECK(tmp.take((void**)&offsets, (size_t)(V + 1) * sizeof(int32_t)));
        if (n_bytes > 0) GTR_CHECK(hipMemcpyAsync(bytes, bytes_host, (size_t)n_bytes, hipMemcpyHostToDevice, stream()));
        GTR_CHECK(hipMemcpyAsync(offsets, offsets_host, (size_t)(V + 1) * sizeof(int32_t), hipMemcpyHostToDevice, stream()));
    }
    GTR_CHECK(hipStreamSynchronize(stream()));
    if (s.vocab_bytes) GTR_CHECK(hipFree(s.vocab_bytes));
    if (s.vocab_offsets) GTR_CHECK(hipFree(s.vocab_offsets));
    tmp.release(bytes);
    tmp.release(offsets);
    s.vocab_bytes = bytes; s.vocab_offsets = offsets; s.vocab_n_bytes = n_bytes;
    return 0;
}

// (the body is gten_hip_decoder_set_fsm_parts_ex's, csrc/gten_fsm_search.h: parts that name the rule their automaton is expanded by)
int gten_hip_decoder_set_fsm_parts(gten_hip_decoder* dc, int n_states, const uint8_t* flags_host, const gten_hip_fsm_part* parts, int n_parts)
{
    std::vector<gten_hip_fsm_part_ex> ex;
    for (int k = 0; parts && k < n_parts; k++) {
        const gten_hip_fsm_part& p = parts[k];
        ex.push_back(gten_hip_fsm_part_ex{p.first, p.count, p.rows_host, p.next256_host, p.accept_host, p.n_byte_states, p.eos, GTEN_HIP_FSM_PART_MATCH});
    }
    return gten_hip_decoder_set_fsm_parts_ex(dc, n_states, flags_host, parts ? ex.data() : nullptr, n_parts);
}

} // extern "C"
