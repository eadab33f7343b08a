// gten_kv_shift.h -- context shift of K / V caches in place (include/gten_hip_shift.h); included by gten_decode.hip
// behind its other entry points.  One kernel, one launch for all (sequence, layer) items of a call:
//
//   k_kv_shift   blockIdx.y is the item.  The first n_stripes workgroups of an item are K's: ONE WAVE owns a stripe of 64 columns
//                (one 64-wide head, or two 32-wide ones) on every moved row; a lane is an element, its rotation partner sits
//                d_head / 2 lanes away, a Q8 block's absmax is a 32-lane reduction.  The other workgroups are V's: a thread owns one
//                piece (16, 4 or 2 bytes, by alignment) of every moved row.
//
// The move overlaps whenever drop < m.  It is race-free by OWNERSHIP, not by any order between workgroups or waves: nobody but its
// owner reads or writes a stripe, the owner walks its rows in ascending order SHIFT_ROWS at a time, and it has loaded rows
// keep + drop + [i0, i0 + SHIFT_ROWS) into registers before it stores rows keep + [i0, i0 + SHIFT_ROWS) -- a later batch reads only
// rows above everything stored so far (drop >= 1).  k_permute_sets' idea (gten_decode_beam.h): load, then store; no barrier, no LDS,
// no second buffer.  SHIFT_ROWS loads are in flight per owner: a stripe of up to 2047 rows is a latency-bound walk otherwise.
#pragma once

#include "gten_hip_shift.h"

static_assert(sizeof(gten_hip_kv_shift_item) == 32, "include/gten_hip_shift.h layout");

#define SHIFT_ROWS 8
// (the cache pointers come out of memory: named global, or the loads and stores would be flat ones)
#define SHIFT_G(T) __attribute__((address_space(1))) T

typedef unsigned shift_u4 __attribute__((ext_vector_type(4)));

// ADT: GTEN_Q8 or GTEN_F16; DH: 32 or 64; VT: V's piece (shift_u4, uint32_t or uint16_t).  grid (n_stripes + V's workgroups, items)
template <int ADT, int DH, typename VT>
__global__ __launch_bounds__(64) void k_kv_shift(const gten_hip_kv_shift_item* __restrict__ items, size_t pitch, int kv_dim, int n_stripes, unsigned n_pieces,
                                                const float2* __restrict__ table)
{
    const gten_hip_kv_shift_item it = items[blockIdx.y];
    const int m = it.n - it.keep - it.drop;
    if (m <= 0) return;                                     // nothing moves, nothing is written (and drop may be past the table)
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= n_stripes) {
        const unsigned p = (blockIdx.x - (unsigned)n_stripes) * 64u + (unsigned)lane;
        if (p >= n_pieces) return;
        const uintptr_t dst = (uintptr_t)it.v + (size_t)it.keep * pitch + (size_t)p * sizeof(VT), src = dst + (size_t)it.drop * pitch;
        for (int i0 = 0; i0 < m; i0 += SHIFT_ROWS) {
            VT t[SHIFT_ROWS];
#pragma unroll
            for (int r = 0; r < SHIFT_ROWS; r++)
                if (i0 + r < m) t[r] = *(const SHIFT_G(VT)*)(src + (size_t)(i0 + r) * pitch);
#pragma unroll
            for (int r = 0; r < SHIFT_ROWS; r++)
                if (i0 + r < m) *(SHIFT_G(VT)*)(dst + (size_t)(i0 + r) * pitch) = t[r];
        }
        return;
    }
    constexpr int HALF = DH / 2;
    const int e = (int)blockIdx.x * 64 + lane;              // this lane's column
    const bool on = e < kv_dim;                             // (kv_dim % DH == 0 and DH divides 64: a lane and its partner are on together)
    const bool hi = (e & HALF) != 0;                        // the second half of its head: v1
    const float2 cs = table[(size_t)it.drop * HALF + (e & (HALF - 1))];
    const size_t at = ADT == GTEN_Q8 ? (size_t)(e >> 5) * GTEN_Q8_BYTES : (size_t)e * 2;         // the block's delta, or the half-word
    const uintptr_t dst = (uintptr_t)it.k + (size_t)it.keep * pitch + at, src = dst + (size_t)it.drop * pitch;
    for (int i0 = 0; i0 < m; i0 += SHIFT_ROWS) {
        uint16_t h[SHIFT_ROWS];                             // the half-word, or the block's delta
        int8_t q[SHIFT_ROWS];
#pragma unroll
        for (int r = 0; r < SHIFT_ROWS; r++) {
            h[r] = 0;
            q[r] = 0;
            if (i0 + r < m && on) {
                const uintptr_t row = src + (size_t)(i0 + r) * pitch;
                h[r] = *(const SHIFT_G(uint16_t)*)row;
                if (ADT == GTEN_Q8) q[r] = *(const SHIFT_G(int8_t)*)(row + 2 + (e & 31));
            }
        }
#pragma unroll
        for (int r = 0; r < SHIFT_ROWS; r++) {
            if (i0 + r >= m) break;                         // (wave-uniform: every lane takes part in the cross-lane steps below)
            const float mine = ADT == GTEN_Q8 ? (float)(int)q[r] * h2f(h[r]) : h2f(h[r]);
            const float other = __shfl_xor(mine, HALF, 64);
            // unrot: v0' = v1 * s + v0 * c (rotary_emb's second output on the swapped row), v1' = v1 * c - v0 * s (its first)
            const float a = mine * cs.x, b = other * cs.y;
            const float y = hi ? a - b : b + a;
            const uintptr_t row = dst + (size_t)(i0 + r) * pitch;
            if (ADT == GTEN_Q8) {
                const Q8Scale sc = q8_scale_from_absmax(nn_max32(fabsf(y)));
                const int qv = q8_round(y, sc.scale);
                if (on) {
                    *(SHIFT_G(int8_t)*)(row + 2 + (e & 31)) = (int8_t)qv;
                    if ((e & 31) == 0) *(SHIFT_G(uint16_t)*)row = sc.d16;
                }
            } else if (on) {
                *(SHIFT_G(uint16_t)*)row = f2h(y);
            }
        }
    }
}

// ---------------------------------------------------------------- host side

static GrowBuf g_shift_items_dev;

template <int ADT, int DH>
static int kv_shift_launch(int vpiece, dim3 grid, const gten_hip_kv_shift_item* items_dev, size_t pitch, int kv_dim, int n_stripes, unsigned n_pieces,
                           const float2* table)
{
    auto kern = vpiece == 16 ? k_kv_shift<ADT, DH, shift_u4> : vpiece == 4 ? k_kv_shift<ADT, DH, uint32_t> : k_kv_shift<ADT, DH, uint16_t>;
    GTR_LAUNCH(KT_PACK, kern, grid, dim3(64), 0, items_dev, pitch, kv_dim, n_stripes, n_pieces, table);
    return 0;
}

extern "C" {

int gten_hip_kv_shift(const gten_hip_kv_shift_item* items_host, int n_items, int adtype, size_t pitch, int kv_dim, int d_head)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(items_host && n_items >= 1, "kv_shift: %d items", n_items);
    GTR_REQUIRE(adtype == GTEN_Q8 || adtype == GTEN_F16, "kv_shift: activation dtype %d (Q8 or F16)", adtype);
    GTR_REQUIRE(d_head == 32 || d_head == 64, "kv_shift: d_head %d (32 or 64)", d_head);
    GTR_REQUIRE(kv_dim >= d_head && kv_dim % d_head == 0 && kv_dim <= 65536, "kv_shift: kv_dim %d is no multiple of d_head %d", kv_dim, d_head);
    const size_t row_bytes = gten_hip_row_bytes(adtype, kv_dim);
    GTR_REQUIRE(pitch >= row_bytes && pitch % 2 == 0, "kv_shift: pitch %zu for rows of %zu bytes (at least that, and even)", pitch, row_bytes);
    // every item is looked at before the first launch: a refused call has written nothing
    int vpiece = pitch % 16 == 0 && row_bytes % 16 == 0 ? 16 : pitch % 4 == 0 && row_bytes % 4 == 0 ? 4 : 2;
    for (int i = 0; i < n_items; i++) {
        const gten_hip_kv_shift_item& it = items_host[i];
        GTR_REQUIRE(it.k && it.v, "kv_shift: item %d has a null cache", i);
        GTR_REQUIRE((uintptr_t)it.k % 2 == 0 && (uintptr_t)it.v % 2 == 0, "kv_shift: item %d: a cache is not 2-byte aligned", i);
        GTR_REQUIRE(it.n >= 0 && it.n <= GTEN_ROPE_MAX_POS, "kv_shift: item %d: %d rows (at most %d: the RoPE table)", i, it.n, GTEN_ROPE_MAX_POS);
        GTR_REQUIRE(it.keep >= 0, "kv_shift: item %d: keep %d is negative", i, it.keep);
        GTR_REQUIRE(it.drop >= 1, "kv_shift: item %d: drop %d (at least 1: there is no no-op form)", i, it.drop);
        GTR_REQUIRE((long long)it.keep + it.drop <= it.n, "kv_shift: item %d: keep %d + drop %d exceed its %d rows", i, it.keep, it.drop, it.n);
        while (vpiece > 2 && (uintptr_t)it.v % (unsigned)vpiece != 0) vpiece = vpiece == 16 ? 4 : 2;
    }
    const float2* table = nullptr;
    if (int rc = rope_table(d_head, &table)) return rc;
    // the records go to the device once per call
    if (int rc = grow_upload(g_shift_items_dev, items_host, (size_t)n_items * sizeof(gten_hip_kv_shift_item))) return rc;
    const int n_stripes = (kv_dim + 63) / 64;
    const unsigned n_pieces = (unsigned)(row_bytes / (size_t)vpiece);
    const gten_hip_kv_shift_item* dev = (const gten_hip_kv_shift_item*)g_shift_items_dev.dev;
    for (int i0 = 0; i0 < n_items; i0 += 65535) {            // (a grid's y extent: one launch unless a call names more items than that)
        const dim3 grid((unsigned)n_stripes + (n_pieces + 63u) / 64u, (unsigned)std::min(n_items - i0, 65535));
        int rc;
        if (adtype == GTEN_Q8) rc = d_head == 64 ? kv_shift_launch<GTEN_Q8, 64>(vpiece, grid, dev + i0, pitch, kv_dim, n_stripes, n_pieces, table)
                                                : kv_shift_launch<GTEN_Q8, 32>(vpiece, grid, dev + i0, pitch, kv_dim, n_stripes, n_pieces, table);
        else rc = d_head == 64 ? kv_shift_launch<GTEN_F16, 64>(vpiece, grid, dev + i0, pitch, kv_dim, n_stripes, n_pieces, table)
                               : kv_shift_launch<GTEN_F16, 32>(vpiece, grid, dev + i0, pitch, kv_dim, n_stripes, n_pieces, table);
        if (rc) return rc;
    }
    // like every other writer of cache rows: [keep, keep + m) of K and V (the last row's pitch padding is not written, nor announced)
    if (kv_watch_any())
        for (int i = 0; i < n_items; i++) {
            const gten_hip_kv_shift_item& it = items_host[i];
            const int m = it.n - it.keep - it.drop;
            if (m <= 0) continue;
            const size_t bytes = (size_t)(m - 1) * pitch + row_bytes;
            kv_watch_touch((const uint8_t*)it.k + (size_t)it.keep * pitch, bytes);
            kv_watch_touch((const uint8_t*)it.v + (size_t)it.keep * pitch, bytes);
        }
    return 0;
}

} // extern "C"
