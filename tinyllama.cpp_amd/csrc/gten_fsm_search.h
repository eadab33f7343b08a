// gten_fsm_search.h -- SEARCH automata over bytes (stop strings given as text) expanded over the vocabulary into the decoder's
// automaton pool, on the device (include/gten_hip_stoptext.h).  Included by gten_decode.hip behind gten_fsm_expand.h,
// whose launch shape, scratch type and pool check it uses.  The definition the expansion is held to, byte for byte, is
// search_expand() of host/regex_build.h.
//
// k_fsm_expand_search is k_fsm_expand with another rule, not a branch inside it: a workgroup takes FX_THREADS consecutive ids -- a
// thread one id -- and GTEN_HIP_FSM_EXPAND_STATES consecutive states; the ids' bytes are staged in LDS GTEN_HIP_FSM_EXPAND_CHUNK at a
// time and walked by GTEN_HIP_FSM_EXPAND_PASS states at a time, held in registers; every store instruction of a wave writes 64
// consecutive u16 of one row.  What differs: the walk never ends at a piece's end in a dead state (the automaton is total), an empty
// piece keeps its state, and each walked state carries one sticky bit, set when the state after a byte is accepting -- the piece then
// enters the HIT state wherever it ends.  The range is always Sb + 1 rows and takes no eos.

// flags[base + s]: 0 for the automaton's states, FINAL for the HIT state behind them
__global__ __launch_bounds__(FX_THREADS) void k_fsm_expand_search_flags(uint8_t* __restrict__ flags, int base, int Sb)
{
    const int s = (int)blockIdx.x * FX_THREADS + (int)threadIdx.x;
    if (s <= Sb) flags[(size_t)base + (size_t)s] = s == Sb ? (uint8_t)GTEN_HIP_FSM_FINAL : (uint8_t)0;
}

// rows [base, base + Sb] of `next`
__global__ __launch_bounds__(FX_THREADS) void k_fsm_expand_search(uint16_t* __restrict__ next, int V, int base, const uint8_t* __restrict__ bytes,
                                                                   long long n_bytes, const int32_t* __restrict__ offsets,
                                                                   const uint16_t* __restrict__ next256, const uint8_t* __restrict__ accept, int Sb)
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
    const int n_rows = Sb + 1;
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
        unsigned hit = 0;                                                               // bit k: walk k has passed an accepting state
#pragma unroll
        for (int k = 0; k < GTEN_HIP_FSM_EXPAND_PASS; k++) cur[k] = s0 + k < Sb ? s0 + k : -1;                    // (the HIT row: dead)
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
                        if (e < Sb && accept[e]) hit |= 1u << k;
                    }
            }
        }
        if (t < V) {
#pragma unroll
            for (int k = 0; k < GTEN_HIP_FSM_EXPAND_PASS; k++) {
                const int s = s0 + k;
                if (s >= s_end) break;
                const uint16_t v = cur[k] < 0 ? (uint16_t)GTEN_HIP_FSM_DEAD : (uint16_t)(base + (((hit >> k) & 1u) ? Sb : cur[k]));
                next[((size_t)base + (size_t)s) * (size_t)V + (size_t)t] = v;
            }
        }
    }
}

namespace {

int fx_launch_search(uint16_t* next_dev, uint8_t* flags_dev, int n_vocab, int base, const uint8_t* bytes, long long n_bytes, const int32_t* offsets,
                     const uint16_t* next256, const uint8_t* accept, int Sb)
{
    const int n_rows = Sb + 1;
    GTR_LAUNCH(KT_DEC_SAMPLE, k_fsm_expand_search_flags, dim3((unsigned)((n_rows + FX_THREADS - 1) / FX_THREADS)), dim3(FX_THREADS), 0, flags_dev, base, Sb);
    const dim3 grid((unsigned)((n_vocab + FX_THREADS - 1) / FX_THREADS), (unsigned)((n_rows + GTEN_HIP_FSM_EXPAND_STATES - 1) / GTEN_HIP_FSM_EXPAND_STATES));
    GTR_LAUNCH(KT_DEC_SAMPLE, k_fsm_expand_search, grid, dim3(FX_THREADS), 0, next_dev, n_vocab, base, bytes, n_bytes, offsets, next256, accept, Sb);
    return 0;
}

} // namespace

extern "C" {

int gten_hip_fsm_expand_search(uint16_t* next_dev, uint8_t* flags_dev, int n_states, int n_vocab, int base, const uint8_t* bytes, long long n_bytes,
                               const int32_t* offsets, const uint16_t* next256, const uint8_t* accept, int n_byte_states)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(next_dev && flags_dev && offsets && next256 && accept && (bytes || n_bytes == 0), "fsm_expand_search: null argument");
    GTR_REQUIRE(n_states >= 1 && n_states <= GTEN_HIP_FSM_MAX_STATES && n_vocab >= 1 && n_vocab <= 65535, "fsm_expand_search: a pool of %d states over %d ids",
                n_states, n_vocab);
    GTR_REQUIRE(n_bytes >= 0 && n_bytes <= 0x7FFFFFFFll, "fsm_expand_search: %lld vocabulary bytes", n_bytes);
    GTR_REQUIRE(n_byte_states >= 1 && base >= 0 && (long long)base + n_byte_states + 1 <= n_states,
                "fsm_expand_search: %d byte states and the HIT state from state %d do not fit the pool's %d", n_byte_states, base, n_states);
    return fx_launch_search(next_dev, flags_dev, n_vocab, base, bytes, n_bytes, offsets, next256, accept, n_byte_states);
}

int gten_hip_decoder_set_fsm_parts_ex(gten_hip_decoder* dc, int n_states, const uint8_t* flags_host, const gten_hip_fsm_part_ex* parts, int n_parts)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_set_fsm_parts: null decoder");
    GTR_REQUIRE(!dc->persist_on, "decoder_set_fsm_parts: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    SamplerState& s = dc->smp;
    GTR_REQUIRE(s.n_fsm == 0, "decoder_set_fsm_parts: %d sequences are bound to the present pool (gten_hip_decoder_set_seq_fsm(.., -1, 0) first)", s.n_fsm);
    const int V = dc->d.n_vocab;
    GTR_REQUIRE(flags_host && parts && n_parts >= 1 && n_states >= 1 && n_states <= GTEN_HIP_FSM_MAX_STATES, "decoder_set_fsm_parts: %d states (1 .. %d), or a null table",
                n_states, GTEN_HIP_FSM_MAX_STATES);
    GTR_REQUIRE((unsigned long long)n_states * (unsigned long long)V * 2ull <= GTEN_HIP_FSM_MAX_BYTES, "decoder_set_fsm_parts: %d states of %d ids are more than %llu bytes",
                n_states, V, (unsigned long long)GTEN_HIP_FSM_MAX_BYTES);
    long long at = 0;
    for (int k = 0; k < n_parts; k++) {
        const gten_hip_fsm_part_ex& p = parts[k];
        GTR_REQUIRE(p.first == at && p.count >= 1 && at + p.count <= n_states, "decoder_set_fsm_parts: part %d covers [%d, %d + %d), expected to start at %lld of %d",
                    k, p.first, p.first, p.count, at, n_states);
        GTR_REQUIRE(p.mode == GTEN_HIP_FSM_PART_MATCH || (p.mode == GTEN_HIP_FSM_PART_SEARCH && !p.rows_host), "decoder_set_fsm_parts: part %d has mode %d", k, p.mode);
        if (!p.rows_host && p.mode == GTEN_HIP_FSM_PART_SEARCH) {
            GTR_REQUIRE(p.next256_host && p.accept_host && p.n_byte_states >= 1 && p.eos == -1 && p.count == p.n_byte_states + 1,
                        "decoder_set_fsm_parts: part %d: a search automaton of %d states with eos %d does not make %d states", k, p.n_byte_states, p.eos, p.count);
        } else if (!p.rows_host) {
            GTR_REQUIRE(p.next256_host && p.accept_host && p.n_byte_states >= 1 && p.eos >= -1 && p.eos < V && p.count == p.n_byte_states + (p.eos >= 0 ? 1 : 0),
                        "decoder_set_fsm_parts: part %d: a byte automaton of %d states with eos %d does not make %d states", k, p.n_byte_states, p.eos, p.count);
        }
        if (!p.rows_host)
            GTR_REQUIRE(s.vocab_offsets, "decoder_set_fsm_parts: part %d is a byte automaton and the decoder has no vocabulary (gten_hip_decoder_set_vocab_bytes)", k);
        at += p.count;
    }
    GTR_REQUIRE(at == n_states, "decoder_set_fsm_parts: the parts cover %lld of %d states", at, n_states);
    GTR_CHECK(hipStreamSynchronize(stream()));             // (no step in flight reads the pool that goes)
    // the new pool is complete and checked on the device before the old one goes: a refusal or a failed allocation leaves the previous pool
    FxScratch tmp;
    uint16_t* next = nullptr;
    uint8_t* flags = nullptr;
    GTR_CHECK(tmp.take((void**)&next, (size_t)n_states * (size_t)V * sizeof(uint16_t)));
    GTR_CHECK(tmp.take((void**)&flags, (size_t)n_states));
    GTR_CHECK(hipMemcpyAsync(flags, flags_host, (size_t)n_states, hipMemcpyHostToDevice, stream()));
    for (int k = 0; k < n_parts; k++) {
        const gten_hip_fsm_part_ex& p = parts[k];
        if (p.rows_host) {
            GTR_CHECK(hipMemcpyAsync(next + (size_t)p.first * (size_t)V, p.rows_host, (size_t)p.count * (size_t)V * sizeof(uint16_t), hipMemcpyHostToDevice, stream()));
            continue;
        }
        uint16_t* n256 = nullptr;
        uint8_t* acc = nullptr;
        GTR_CHECK(tmp.take((void**)&n256, (size_t)p.n_byte_states * 256 * sizeof(uint16_t)));
        GTR_CHECK(tmp.take((void**)&acc, (size_t)p.n_byte_states));
        GTR_CHECK(hipMemcpyAsync(n256, p.next256_host, (size_t)p.n_byte_states * 256 * sizeof(uint16_t), hipMemcpyHostToDevice, stream()));
        GTR_CHECK(hipMemcpyAsync(acc, p.accept_host, (size_t)p.n_byte_states, hipMemcpyHostToDevice, stream()));
        const int rc = p.mode == GTEN_HIP_FSM_PART_SEARCH
                           ? fx_launch_search(next, flags, V, p.first, s.vocab_bytes, s.vocab_n_bytes, s.vocab_offsets, n256, acc, p.n_byte_states)
                           : fx_launch(next, flags, V, p.first, s.vocab_bytes, s.vocab_n_bytes, s.vocab_offsets, n256, acc, p.n_byte_states, p.eos);
        if (rc) return rc;
    }
    int bad = 0;
    long long where = -1;
    if (const int rc = fx_check(next, flags, n_states, V, &bad, &where)) return rc;
    GTR_REQUIRE(bad != GTEN_HIP_FSM_BAD_ENTRY, "decoder_set_fsm_parts: state %lld has an entry that is neither a state nor DEAD", where);
    GTR_REQUIRE(bad != GTEN_HIP_FSM_STUCK, "decoder_set_fsm_parts: state %lld is not final and allows no id", where);
    std::vector<uint8_t> flags_now((size_t)n_states);
    GTR_CHECK(hipMemcpy(flags_now.data(), flags, (size_t)n_states, hipMemcpyDeviceToHost));      // (the expanded ranges' flags were made on the device)
    // (the pool's pointers and size are arguments of the captured step-end launch: graphs that hold the old ones go)
    if (s.fsm_on) GTR_CHECK(drop_graphs(dc));
    if (s.fsm_next) GTR_CHECK(hipFree(s.fsm_next));
    if (s.fsm_flags) GTR_CHECK(hipFree(s.fsm_flags));
    tmp.release(next);
    tmp.release(flags);
    s.fsm_next = next; s.fsm_flags = flags; s.fsm_states = n_states;
    s.fsm_flags_host.swap(flags_now);
    return 0;
}

} // extern "C"
