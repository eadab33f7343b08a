// gten_decode_beam.h -- beam search on the device (include/gten_hip_beam.h); included by gten_decode.hip behind its
// other entry points.  Two kernels and the decoder form that strings them behind a shared step:
//
//   k_beam_round    one wave per group.  The group's at most 8 x 16 candidates go into LDS, every candidate counts how many
//                   precede it under (score descending, beam ascending, rank ascending) -- its place, an integer fact --, the
//                   first 2B are written in order and lane 0 walks them: at most 16 serial steps, no float sum anywhere.
//   k_permute_sets  a thread owns one piece: the same offset in all B sets of a range.  It loads the piece from every set that
//                   moves, then stores: nobody else touches that offset, so the gather is in place without a barrier, LDS or a
//                   second buffer.  Plain vector loads and stores.
//
// The decoder form takes the lists from the step's own records (a log-prob request of n_top = 2B on the group's sequences, §3.11):
// the round reads them where the sampler launch left them and writes the chosen ids into the sequences' token rows.
#pragma once

#include "gten_hip_beam.h"

static_assert(2 * GTEN_HIP_BEAM_MAX <= GTEN_HIP_LOGPROBS_TOP, "a beam's candidate list is one log-prob record");
static_assert(sizeof(gten_hip_beam_state) == 176 && sizeof(gten_hip_permute_range) == 72 && sizeof(gten_hip_beam_group) == 20, "include/gten_hip_beam.h layouts");

#define BEAM_B GTEN_HIP_BEAM_MAX
#define BEAM_CAND (BEAM_B * 2 * BEAM_B)          // 128 candidates at most
#define PERMUTE_THREADS 256

// Where a round finds its lists and leaves its ids.  List row of beam b at round t (the new t):
//   top_id + (row0 + b) * row_stride + (pos0 + t - 1) * pos_step, top_lp alike; next_id + (row0 + b) * next_stride + (pos0 + t - 1) * next_step
// with pos0 = prompt_len where pos_step != 0.  The operator: pos_step = next_step = 0, next_stride = 1.  The decoder: the lists are
// the records [sequence][position] (strides in 4-byte words), the ids go into the token rows.
struct BeamIo {
    const int32_t* top_id; const float* top_lp;
    long long row_stride; int pos_step;
    int32_t* next_id; int next_stride, next_step;
};

__global__ __launch_bounds__(64) void k_beam_round(const gten_hip_beam_group* __restrict__ groups, gten_hip_beam_state* __restrict__ state, BeamIo io,
                                                  const float* __restrict__ w, int n_w, int32_t* __restrict__ parent, int32_t* __restrict__ ids, int trellis_rows)
{
    __shared__ float c_score[BEAM_CAND];
    __shared__ float s_score[2 * BEAM_B];
    __shared__ int s_b[2 * BEAM_B], s_id[2 * BEAM_B];
    const int g = blockIdx.x, lane = threadIdx.x;
    const gten_hip_beam_group grp = groups[g];
    gten_hip_beam_state* st = state + g;
    const int B = grp.n_beams;
    if (B < 1 || B > BEAM_B) return;
    if (io.pos_step == 0 && io.row_stride < 2 * B) return;  // (the operator's lists would overlap: the group is left alone)
    const int t = st->t + 1;
    if (st->done) return;                                   // (not one byte of a done group changes)
    if (t > grp.max_new || t >= trellis_rows || t >= n_w) { // out of rounds: left alone, and the gather must not repeat the last one
        if (lane == 0) st->stepped = 0;
        return;
    }
    const int L = 2 * B, n_src = t == 1 ? 1 : B, n_cand = n_src * L;
    const long long pos = io.pos_step ? (long long)(grp.prompt_len + t - 1) : 0;
    // candidates c = b * L + r: (beam ascending, rank ascending) is index ascending
    int my_id[2];
    float my_score[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int c = lane + 64 * k;
        my_id[k] = -1;
        my_score[k] = 0.f;
        if (c < n_cand) {
            const int b = c / L, r = c - b * L;
            const long long at = (long long)(grp.row0 + b) * io.row_stride + pos * io.pos_step + r;
            my_id[k] = io.top_id[at];
            my_score[k] = st->cum[b] + io.top_lp[at];
            c_score[c] = my_score[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int c = lane + 64 * k;
        if (c >= n_cand) continue;
        int place = 0;
        for (int j = 0; j < n_cand; j++) {
            const float sj = c_score[j];
            place += (int)(sj > my_score[k] || (sj == my_score[k] && j < c));
        }
        if (place < L) { s_score[place] = my_score[k]; s_b[place] = c / L; s_id[place] = my_id[k]; }
    }
    __syncthreads();
    if (lane != 0) return;
    const float wt = w[t];
    int32_t* prow = parent + ((size_t)g * trellis_rows + t) * BEAM_B;
    int32_t* irow = ids + ((size_t)g * trellis_rows + t) * BEAM_B;
    int n_next = 0, n_fin = st->n_fin;
    const int n_walk = min(L, n_cand);
    for (int k = 0; k < n_walk && n_next < B; k++) {
        const float score = s_score[k];
        const int b = s_b[k], id = s_id[k];
        if (grp.eos >= 0 && id == grp.eos) {
            if (k >= B) continue;
            const float fin = score * wt;
            int slot = -1;
            if (n_fin < B) slot = n_fin++;
            else {
                int lo = 0;
                for (int j = 1; j < B; j++)
                    if (st->fin_final[j] <= st->fin_final[lo]) lo = j;      // the smallest, ties to the highest slot
                if (fin > st->fin_final[lo]) slot = lo;
            }
            if (slot >= 0) { st->fin_final[slot] = fin; st->fin_cum[slot] = score; st->fin_t[slot] = t; st->fin_beam[slot] = b; }
        } else {
            prow[n_next] = b;
            irow[n_next] = id;
            st->cum[n_next] = score;                        // (every candidate's score was formed before the barrier)
            io.next_id[(long long)(grp.row0 + n_next) * io.next_stride + pos * io.next_step] = id;
            n_next++;
        }
    }
    st->n_fin = n_fin;
    st->done = n_fin >= B ? 1 : 0;
    st->t = t;
    st->stepped = 1;
}

// groups not done, by one wave
__global__ __launch_bounds__(64) void k_beam_live(const gten_hip_beam_state* __restrict__ state, int n_groups, int32_t* __restrict__ out)
{
    int n = 0;
    for (int g = threadIdx.x; g < n_groups; g += 64) n += state[g].done ? 0 : 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (threadIdx.x == 0) out[0] = n;
}

typedef unsigned permute_u4 __attribute__((ext_vector_type(4)));
// T: permute_u4 (16-byte pieces) or uint32_t.  grid (pieces / PERMUTE_THREADS, ranges)
template <typename T>
__global__ __launch_bounds__(PERMUTE_THREADS) void k_permute_sets(const gten_hip_permute_range* __restrict__ ranges, size_t offset, unsigned n_pieces,
                                                                  const gten_hip_beam_group* __restrict__ groups, const gten_hip_beam_state* __restrict__ state,
                                                                  const int32_t* __restrict__ parent, int trellis_rows)
{
    const gten_hip_permute_range* rg = ranges + blockIdx.y;
    const int g = rg->group;
    const int B = groups[g].n_beams;
    if (B < 1 || B > BEAM_B) return;
    const int32_t* prow = parent + (size_t)g * BEAM_B;
    if (state) {
        const gten_hip_beam_state* st = state + g;
        if (st->done || !st->stepped || st->t < 0 || st->t >= trellis_rows) return;        // (workgroup-uniform)
        prow = parent + ((size_t)g * trellis_rows + st->t) * BEAM_B;
    }
    // (named scalars, not arrays indexed in loops: every piece stays in registers)
#define PERMUTE_EACH(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define PERMUTE_SRC(b) int s##b = b < B ? prow[b] : b; if (s##b < 0 || s##b >= B) s##b = b;
    PERMUTE_EACH(PERMUTE_SRC)
#define PERMUTE_MOVES(b) || s##b != b
    if (!(false PERMUTE_EACH(PERMUTE_MOVES))) return;       // the identity: nothing moves (workgroup-uniform)
    const unsigned i = blockIdx.x * PERMUTE_THREADS + threadIdx.x;
    if (i >= n_pieces) return;
    // (the bases come out of memory: named global, or the loads and stores would be flat ones)
#define PERMUTE_LOAD(b) T v##b = T(); if (s##b != b) v##b = ((const __attribute__((address_space(1))) T*)((uintptr_t)rg->base[s##b] + offset))[i];
    PERMUTE_EACH(PERMUTE_LOAD)
#define PERMUTE_STORE(b) if (s##b != b) ((__attribute__((address_space(1))) T*)((uintptr_t)rg->base[b] + offset))[i] = v##b;
    PERMUTE_EACH(PERMUTE_STORE)
#undef PERMUTE_STORE
#undef PERMUTE_LOAD
#undef PERMUTE_MOVES
#undef PERMUTE_SRC
#undef PERMUTE_EACH
}

// ---------------------------------------------------------------- host side

static int beam_round_launch(const gten_hip_beam_group* groups, int n_groups, gten_hip_beam_state* state, const BeamIo& io, const float* w, int n_w,
                             int32_t* parent, int32_t* ids, int trellis_rows)
{
    GTR_LAUNCH(KT_DEC_SAMPLE, k_beam_round, dim3(n_groups), dim3(64), 0, groups, state, io, w, n_w, parent, ids, trellis_rows);
    return 0;
}

static int permute_launch(const gten_hip_permute_range* ranges_dev, int n_ranges, size_t offset, size_t bytes, bool wide, const gten_hip_beam_group* groups,
                          const gten_hip_beam_state* state, const int32_t* parent, int trellis_rows)
{
    const size_t piece = wide ? 16 : 4, n_pieces = bytes / piece;
    const dim3 grid((unsigned)((n_pieces + PERMUTE_THREADS - 1) / PERMUTE_THREADS), (unsigned)n_ranges);
    if (wide)
        GTR_LAUNCH(KT_PACK, k_permute_sets<permute_u4>, grid, dim3(PERMUTE_THREADS), 0, ranges_dev, offset, (unsigned)n_pieces, groups, state, parent, trellis_rows);
    else
        GTR_LAUNCH(KT_PACK, k_permute_sets<uint32_t>, grid, dim3(PERMUTE_THREADS), 0, ranges_dev, offset, (unsigned)n_pieces, groups, state, parent, trellis_rows);
    return 0;
}

// what a decoder keeps of a search between begin and end
struct BeamSearch {
    std::vector<gten_hip_beam_group> groups;
    std::vector<int> lp_before;                 // per sequence of a group: its log-prob request before begin
    gten_hip_beam_group* groups_dev = nullptr;
    gten_hip_beam_state* state = nullptr;
    int32_t *parent = nullptr, *ids = nullptr, *live = nullptr;
    float* w = nullptr;
    gten_hip_permute_range* ranges = nullptr;
    int n_w = 0, trellis_rows = 0, n_ranges = 0, rounds = 0, max_rounds = 0;
    size_t kv_pitch = 0;
    bool wide = false;
    bool on = false;
    unsigned long long permute_bytes = 0, permute_launches = 0;
};

static hipError_t beam_free(BeamSearch* bs)
{
    hipError_t first = hipSuccess;
    if (!bs) return first;
    for (void* p : {(void*)bs->groups_dev, (void*)bs->state, (void*)bs->parent, (void*)bs->ids, (void*)bs->live, (void*)bs->w, (void*)bs->ranges})
        if (p) { const hipError_t e = hipFree(p); if (e != hipSuccess && first == hipSuccess) first = e; }
    bs->groups_dev = nullptr; bs->state = nullptr; bs->parent = bs->ids = bs->live = nullptr; bs->w = nullptr; bs->ranges = nullptr;
    return first;
}
static hipError_t beam_destroy(gten_hip_decoder* dc)
{
    const hipError_t e = beam_free(dc->beam);
    delete dc->beam;
    dc->beam = nullptr;
    return e;
}

static GrowBuf g_permute_ranges_dev;

// the log-prob requests of the groups' sequences in one upload and one wait: n_top[i] for the i-th sequence of the groups in order
// (-1: none).  The decoder's first request ever goes through first_use, as gten_hip_decoder_set_logprobs' does.
static int beam_requests(gten_hip_decoder* dc, const std::vector<gten_hip_beam_group>& groups, const std::vector<int>& n_top)
{
    bool any = false;
    for (int v : n_top) any = any || v >= 0;
    if (any && !dc->smp.lp_on)
        if (int rc = first_use(dc, dc->smp.lp_on, lp_make)) return rc;
    size_t i = 0;
    for (const gten_hip_beam_group& G : groups)
        for (int q = G.row0; q < G.row0 + G.n_beams; q++, i++) {
            SampleParam& p = dc->smp.samp_host[(size_t)q];
            dc->smp.n_asking += (n_top[i] >= 0 ? 1 : 0) - (p.lp1 > 0u ? 1 : 0);
            p.lp1 = (unsigned)(n_top[i] + 1);
        }
    GTR_CHECK(hipMemcpyAsync(dc->smp.samp, dc->smp.samp_host.data(), dc->smp.samp_host.size() * sizeof(SampleParam), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    return 0;
}

extern "C" {

int gten_hip_beam_round(const gten_hip_beam_group* groups, int n_groups, gten_hip_beam_state* state, const int32_t* top_id, const float* top_lp,
                        long long row_stride, const float* w, int n_w, int32_t* parent, int32_t* ids, int trellis_rows, int32_t* next_id)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(groups && state && top_id && top_lp && w && parent && ids && next_id, "beam_round: null argument");
    GTR_REQUIRE(n_groups >= 1 && n_groups <= 65535, "beam_round: %d groups outside [1, 65535]", n_groups);
    GTR_REQUIRE(row_stride >= 2 && n_w >= 2 && trellis_rows >= 2, "beam_round: row_stride %lld, %d weights, %d trellis rows (each at least 2)", row_stride, n_w,
                trellis_rows);
    const BeamIo io{top_id, top_lp, row_stride, 0, next_id, 1, 0};
    return beam_round_launch(groups, n_groups, state, io, w, n_w, parent, ids, trellis_rows);
}

int gten_hip_permute_sets(const gten_hip_permute_range* ranges_host, int n_ranges, size_t offset, size_t bytes, const gten_hip_beam_group* groups,
                          int n_groups, const gten_hip_beam_state* state, const int32_t* parent, int trellis_rows)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(ranges_host && groups && parent, "permute_sets: null argument");
    GTR_REQUIRE(n_ranges >= 1 && n_ranges <= 65535 && n_groups >= 1, "permute_sets: %d ranges outside [1, 65535], %d groups", n_ranges, n_groups);
    GTR_REQUIRE(bytes % 4 == 0 && offset % 4 == 0, "permute_sets: offset %zu, %zu bytes (multiples of 4)", offset, bytes);
    GTR_REQUIRE(bytes / 4 <= 0xffffffffull, "permute_sets: %zu bytes", bytes);
    GTR_REQUIRE(!state || trellis_rows >= 1, "permute_sets: %d trellis rows", trellis_rows);
    if (bytes == 0) return 0;
    bool wide = offset % 16 == 0 && bytes % 16 == 0;
    for (int i = 0; i < n_ranges; i++) {
        const gten_hip_permute_range& r = ranges_host[i];
        GTR_REQUIRE(r.group >= 0 && r.group < n_groups, "permute_sets: range %d names group %d outside [0, %d)", i, r.group, n_groups);
        for (int b = 0; b < GTEN_HIP_BEAM_MAX; b++) {
            if (!r.base[b]) continue;                       // (sets past the group's n_beams)
            GTR_REQUIRE((uintptr_t)r.base[b] % 4 == 0, "permute_sets: range %d, base %d is not 4-byte aligned", i, b);
            wide = wide && (uintptr_t)r.base[b] % 16 == 0;
            kv_watch_touch((const uint8_t*)r.base[b] + offset, bytes);
        }
    }
    if (int rc = grow_upload(g_permute_ranges_dev, ranges_host, (size_t)n_ranges * sizeof(gten_hip_permute_range))) return rc;
    return permute_launch((const gten_hip_permute_range*)g_permute_ranges_dev.dev, n_ranges, offset, bytes, wide, groups, state, parent, trellis_rows);
}

int gten_hip_decoder_beam_begin(gten_hip_decoder* dc, const gten_hip_beam_group* groups_host, int n_groups, const float* w_host, int n_w)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && groups_host && w_host && n_groups >= 1, "decoder_beam_begin: bad arguments");
    GTR_REQUIRE(!dc->persist_on, "decoder_beam_begin: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    GTR_REQUIRE(dc->n_seq > 1, "decoder_beam_begin: a multi-sequence decoder (gten_hip_decoder_create_multi)");
    GTR_REQUIRE(!dc->beam || !dc->beam->on, "decoder_beam_begin: a search is already begun (gten_hip_decoder_beam_end)");
    const gten_hip_decoder_desc& d = dc->d;
    std::vector<char> taken((size_t)dc->n_seq, 0);
    int max_new_all = 0, min_new = 0x7fffffff;
    for (int g = 0; g < n_groups; g++) {
        const gten_hip_beam_group& G = groups_host[g];
        GTR_REQUIRE(G.n_beams >= 1 && G.n_beams <= GTEN_HIP_BEAM_MAX, "decoder_beam_begin: group %d has %d beams, outside [1, %d]", g, G.n_beams, GTEN_HIP_BEAM_MAX);
        GTR_REQUIRE(G.row0 >= 0 && G.row0 + G.n_beams <= dc->n_seq, "decoder_beam_begin: group %d takes sequences [%d, %d) of %d", g, G.row0, G.row0 + G.n_beams,
                    dc->n_seq);
        GTR_REQUIRE(G.prompt_len >= 1 && G.max_new >= 1 && (long long)G.prompt_len + G.max_new <= d.max_ctx,
                    "decoder_beam_begin: group %d: a prompt of %d ids and %d new ones do not fit max_ctx %d", g, G.prompt_len, G.max_new, d.max_ctx);
        GTR_REQUIRE(2 * G.n_beams <= d.n_vocab, "decoder_beam_begin: group %d: 2 x %d beams exceed the vocabulary of %d ids", g, G.n_beams, d.n_vocab);
        GTR_REQUIRE(G.max_new < n_w, "decoder_beam_begin: group %d: max_new %d needs %d length weights, %d given", g, G.max_new, G.max_new + 1, n_w);
        GTR_REQUIRE(G.eos >= -1 && G.eos < d.n_vocab, "decoder_beam_begin: group %d: eos %d outside [-1, %d)", g, G.eos, d.n_vocab);
        for (int q = G.row0; q < G.row0 + G.n_beams; q++) {
            GTR_REQUIRE(!taken[(size_t)q], "decoder_beam_begin: sequence %d is in two groups", q);
            taken[(size_t)q] = 1;
            const SampleParam& p = dc->smp.samp_host[(size_t)q];
            GTR_REQUIRE(p.top_k == 0, "decoder_beam_begin: sequence %d is sampling (gten_hip_decoder_set_sampling)", q);
            GTR_REQUIRE(p.table1 == 0, "decoder_beam_begin: sequence %d is bound to a bias table (gten_hip_decoder_set_seq_bias)", q);
            GTR_REQUIRE(!fsm_bound(dc, q), "decoder_beam_begin: sequence %d is bound to an automaton (gten_hip_decoder_set_seq_fsm)", q);
            GTR_REQUIRE(!dc->smp.pen_on || dc->smp.pen_host[(size_t)q].on == 0u, "decoder_beam_begin: sequence %d is penalised (gten_hip_decoder_set_penalty)", q);
        }
        max_new_all = std::max(max_new_all, G.max_new);
        min_new = std::min(min_new, G.max_new);
    }
    GTR_REQUIRE((size_t)n_groups * d.n_layers * 2 <= 65535, "decoder_beam_begin: %d groups x %d layers", n_groups, d.n_layers);
    if (!dc->beam) dc->beam = new BeamSearch;
    BeamSearch& bs = *dc->beam;
    GTR_CHECK(hipStreamSynchronize(stream()));
    GTR_CHECK(beam_free(&bs));
    bs.groups.assign(groups_host, groups_host + n_groups);
    bs.n_w = n_w;
    bs.trellis_rows = max_new_all + 1;
    bs.max_rounds = min_new;
    bs.rounds = 0;
    bs.kv_pitch = gten_hip_row_bytes(d.adtype, (d.n_embd / d.n_heads) * d.n_kv_heads);
    // the range tables: per group and layer one range for K and one for V, the bases at the first row the beams write themselves
    std::vector<gten_hip_permute_range> ranges;
    bs.wide = bs.kv_pitch % 16 == 0;
    for (int g = 0; g < n_groups; g++) {
        const gten_hip_beam_group& G = bs.groups[(size_t)g];
        for (int l = 0; l < d.n_layers; l++)
            for (int kv = 0; kv < 2; kv++) {
                gten_hip_permute_range r{};
                r.group = g;
                for (int b = 0; b < G.n_beams; b++) {
                    const uint8_t* cache = (const uint8_t*)dc->kv_real[((size_t)(G.row0 + b) * d.n_layers + l) * 2 + kv];
                    r.base[b] = (void*)(cache + (size_t)(G.prompt_len - 1) * bs.kv_pitch);
                    bs.wide = bs.wide && (uintptr_t)r.base[b] % 16 == 0;
                    GTR_REQUIRE((uintptr_t)r.base[b] % 4 == 0, "decoder_beam_begin: a cache row of sequence %d is not 4-byte aligned", G.row0 + b);
                }
                ranges.push_back(r);
            }
    }
    bs.n_ranges = (int)ranges.size();
    const size_t trellis_bytes = (size_t)n_groups * bs.trellis_rows * BEAM_B * sizeof(int32_t);
    GTR_CHECK(hipMalloc((void**)&bs.groups_dev, (size_t)n_groups * sizeof(gten_hip_beam_group)));
    GTR_CHECK(hipMalloc((void**)&bs.state, (size_t)n_groups * sizeof(gten_hip_beam_state)));
    GTR_CHECK(hipMalloc((void**)&bs.parent, trellis_bytes));
    GTR_CHECK(hipMalloc((void**)&bs.ids, trellis_bytes));
    GTR_CHECK(hipMalloc((void**)&bs.live, sizeof(int32_t)));
    GTR_CHECK(hipMalloc((void**)&bs.w, (size_t)n_w * sizeof(float)));
    GTR_CHECK(hipMalloc((void**)&bs.ranges, ranges.size() * sizeof(gten_hip_permute_range)));
    GTR_CHECK(hipMemcpyAsync(bs.groups_dev, bs.groups.data(), (size_t)n_groups * sizeof(gten_hip_beam_group), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipMemsetAsync(bs.state, 0, (size_t)n_groups * sizeof(gten_hip_beam_state), stream()));
    GTR_CHECK(hipMemsetAsync(bs.parent, 0, trellis_bytes, stream()));
    GTR_CHECK(hipMemsetAsync(bs.ids, 0, trellis_bytes, stream()));
    GTR_CHECK(hipMemcpyAsync(bs.w, w_host, (size_t)n_w * sizeof(float), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipMemcpyAsync(bs.ranges, ranges.data(), ranges.size() * sizeof(gten_hip_permute_range), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));              // (`ranges` lives on this stack frame)
    // the sequences' requests: remembered, then n_top = 2B.  Every other sequence idles as a parked slot does.
    bs.lp_before.clear();
    std::vector<int> asked;
    for (const gten_hip_beam_group& G : bs.groups)
        for (int q = G.row0; q < G.row0 + G.n_beams; q++) {
            bs.lp_before.push_back((int)dc->smp.samp_host[(size_t)q].lp1 - 1);
            asked.push_back(2 * G.n_beams);
        }
    std::vector<int> seqs((size_t)dc->n_seq), n_first((size_t)dc->n_seq, 0), n_last((size_t)dc->n_seq, 0);
    for (int q = 0; q < dc->n_seq; q++) seqs[(size_t)q] = q;
    for (const gten_hip_beam_group& G : bs.groups)
        for (int q = G.row0; q < G.row0 + G.n_beams; q++) n_first[(size_t)q] = G.prompt_len;
    int rc = beam_requests(dc, bs.groups, asked);
    if (!rc) rc = gten_hip_decoder_slots_apply(dc, dc->n_seq, seqs.data(), n_first.data(), n_last.data(), nullptr);
    if (rc) {                                               // nothing begun: the requests are what they were (the first failure is reported)
        beam_requests(dc, bs.groups, bs.lp_before);
        return rc;
    }
    bs.on = true;
    return 0;
}

int gten_hip_decoder_beam_round(gten_hip_decoder* dc)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && dc->beam && dc->beam->on, "decoder_beam_round: no search begun (gten_hip_decoder_beam_begin)");
    BeamSearch& bs = *dc->beam;
    GTR_REQUIRE(bs.rounds < bs.max_rounds, "decoder_beam_round: the %d rounds of the shortest group are over", bs.max_rounds);
    if (int rc = gten_hip_decoder_run(dc, 1)) return rc;
    const int n_groups = (int)bs.groups.size(), rec_words = (int)(sizeof(LpRecord) / 4), rec_stride = dc->d.max_ctx + 2;
    const int32_t* rec = (const int32_t*)dc->smp.lp;
    const BeamIo io{rec + offsetof(LpRecord, top_id) / 4, (const float*)rec + offsetof(LpRecord, top_logprob) / 4, (long long)rec_stride * rec_words, rec_words,
                    dc->tokens, dc->d.max_ctx + 1, 1};
    if (int rc = beam_round_launch(bs.groups_dev, n_groups, bs.state, io, bs.w, bs.n_w, bs.parent, bs.ids, bs.trellis_rows)) return rc;
    bs.rounds++;
    // Round 1 moves nothing: every beam computed row prompt_len - 1 from the same ids behind the same rows, so the B sets hold the same
    // bytes there whatever `parent` says (all groups begin together: rounds == 1 is t == 1 for each) -- no launch, no re-import.
    if (bs.rounds == 1) return 0;
    // the rows the beams wrote themselves: [prompt_len - 1, prompt_len - 1 + rounds) behind every base.  Every set of every group is
    // announced: the host does not know `parent`
    const size_t bytes = (size_t)bs.rounds * bs.kv_pitch;
    if (kv_watch_any())
        for (const gten_hip_beam_group& G : bs.groups)
            for (int b = 0; b < G.n_beams; b++)
                for (int i = 0; i < dc->d.n_layers * 2; i++)
                    kv_watch_touch((const uint8_t*)dc->kv_real[(size_t)(G.row0 + b) * dc->d.n_layers * 2 + i] + (size_t)(G.prompt_len - 1) * bs.kv_pitch, bytes);
    if (int rc = permute_launch(bs.ranges, bs.n_ranges, 0, bytes, bs.wide, bs.groups_dev, bs.state, bs.parent, bs.trellis_rows)) return rc;
    bs.permute_bytes = (unsigned long long)bytes * (unsigned long long)bs.lp_before.size() * (unsigned long long)dc->d.n_layers * 2ull;
    bs.permute_launches++;
    return 0;
}

int gten_hip_decoder_beam_live(gten_hip_decoder* dc, int* n_live)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && n_live && dc->beam && dc->beam->on, "decoder_beam_live: no search begun (gten_hip_decoder_beam_begin)");
    BeamSearch& bs = *dc->beam;
    GTR_LAUNCH(KT_DEC_SAMPLE, k_beam_live, dim3(1), dim3(64), 0, (const gten_hip_beam_state*)bs.state, (int)bs.groups.size(), bs.live);
    int32_t n = 0;
    GTR_CHECK(hipMemcpyAsync(&n, bs.live, sizeof(n), hipMemcpyDeviceToHost, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    *n_live = n;
    return 0;
}

int gten_hip_decoder_beam_read(gten_hip_decoder* dc, int g, gten_hip_beam_state* state_host, int32_t* parent_host, int32_t* ids_host)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && dc->beam && dc->beam->on, "decoder_beam_read: no search begun (gten_hip_decoder_beam_begin)");
    BeamSearch& bs = *dc->beam;
    GTR_REQUIRE(g >= 0 && g < (int)bs.groups.size() && state_host, "decoder_beam_read: group %d outside [0, %zu)", g, bs.groups.size());
    GTR_CHECK(hipMemcpyAsync(state_host, bs.state + g, sizeof(gten_hip_beam_state), hipMemcpyDeviceToHost, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    const int t = std::min(std::max(state_host->t, 0), bs.trellis_rows - 1);
    const size_t at = ((size_t)g * bs.trellis_rows + 1) * BEAM_B;
    if (t > 0 && parent_host) GTR_CHECK(hipMemcpyAsync(parent_host, bs.parent + at, (size_t)t * BEAM_B * 4, hipMemcpyDeviceToHost, stream()));
    if (t > 0 && ids_host) GTR_CHECK(hipMemcpyAsync(ids_host, bs.ids + at, (size_t)t * BEAM_B * 4, hipMemcpyDeviceToHost, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    return 0;
}

int gten_hip_decoder_beam_end(gten_hip_decoder* dc)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && dc->beam && dc->beam->on, "decoder_beam_end: no search begun (gten_hip_decoder_beam_begin)");
    BeamSearch& bs = *dc->beam;
    GTR_CHECK(hipStreamSynchronize(stream()));
    // the requests as they were, and every slot parked: one upload and one wait each
    if (int rc = beam_requests(dc, bs.groups, bs.lp_before)) return rc;
    std::vector<int> seqs, zero;
    for (const gten_hip_beam_group& G : bs.groups)
        for (int q = G.row0; q < G.row0 + G.n_beams; q++) seqs.push_back(q);
    zero.assign(seqs.size(), 0);
    if (int rc = gten_hip_decoder_slots_apply(dc, (int)seqs.size(), seqs.data(), zero.data(), zero.data(), nullptr)) return rc;
    bs.on = false;                                          // (only now: a failed restore leaves the search begun, `end` can be called again)
    GTR_CHECK(beam_free(&bs));
    return 0;
}

int gten_hip_decoder_beam_info(gten_hip_decoder* dc, int* rounds, unsigned long long* permute_bytes, unsigned long long* permute_launches)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_beam_info: null decoder");
    if (rounds) *rounds = dc->beam ? dc->beam->rounds : 0;
    if (permute_bytes) *permute_bytes = dc->beam ? dc->beam->permute_bytes : 0;
    if (permute_launches) *permute_launches = dc->beam ? dc->beam->permute_launches : 0;
    return 0;
}

} // extern "C"
