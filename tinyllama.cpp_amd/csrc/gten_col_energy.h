// gten_col_energy.h -- k_col_energy_partials and k_col_energy_add, the kernels of gten_hip_calib_col_energy
// (include/gten_hip_calib.h, which states what they compute): per column, the sum over activation rows of the squared element, in
// f64, added to an accumulator the caller owns.  Included by gten_ops.hip.  The structure is that of the pooling kernels
//  for the same two storage forms, repeated here so that this header stands alone: one wave per (chunk of
// CE_CHUNK = 64 rows, tile of CE_TILE = 256 columns), a row's bytes fetched as ALIGNED 16-byte requests into LDS and taken apart
// there (a Q8 quant and its block's delta are only 2-byte aligned in a row, and a row starts wherever the pitch puts it; a request
// is issued only where it overlaps a byte that is needed, so it never leaves the 4 KB page of a byte the caller owns).
// DESIGN.md 3.28.
//
// Deterministic without atomics: lane l owns columns 4 l .. 4 l + 3 of the tile and adds the chunk's rows in ascending order from
// +0 (every term is >= +0); the chunk sums go to a library-owned f64 scratch [chunks][cols], and k_col_energy_add -- one
// workgroup per tile of 256 columns, one column per thread -- adds them to acc in ascending chunk order.
#pragma once

#include "gten_dev.h"
#include "gten_rt.h"
#include "../../include/gten_hip_calib.h"

namespace {
constexpr int CE_CHUNK = 64;          // rows of a chunk (the definition's)
constexpr int CE_STEP = 16;           // rows staged in LDS at a time
constexpr int CE_TILE = 256;          // columns of a workgroup of k_col_energy_partials: 4 per lane

// columns c0 .. c0 + 3 (c0 % 4 == 0) of the row bytes at p (2-byte aligned, column 0's block first) as f32
template <int DT> struct EnergyFmt;
template <> struct EnergyFmt<GTEN_Q8> {
    static constexpr int TILE_BYTES = CE_TILE / GTEN_QBLK * GTEN_Q8_BYTES;     // 272
    __device__ static size_t col_byte(int c) { return (size_t)(c / GTEN_QBLK) * GTEN_Q8_BYTES; }           // c % 32 == 0
    __device__ static void load4(const uint8_t* p, int c0, float* v)
    {
        const uint8_t* b = p + (c0 >> 5) * GTEN_Q8_BYTES;
        const float d = gtd::h2f(*reinterpret_cast<const uint16_t*>(b));
        const uint16_t* q = reinterpret_cast<const uint16_t*>(b + 2 + (c0 & 31));
        const uint16_t lo = q[0], hi = q[1];
        v[0] = d * (float)(int8_t)(lo & 0xff);
        v[1] = d * (float)(int8_t)(lo >> 8);
        v[2] = d * (float)(int8_t)(hi & 0xff);
        v[3] = d * (float)(int8_t)(hi >> 8);
    }
};
template <> struct EnergyFmt<GTEN_F16> {
    static constexpr int TILE_BYTES = CE_TILE * 2;                             // 512
    __device__ static size_t col_byte(int c) { return (size_t)c * 2; }
    __device__ static void load4(const uint8_t* p, int c0, float* v)
    {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p) + c0;
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = gtd::h2f(h[i]);
    }
};
} // namespace

template <int DT>
__global__ __launch_bounds__(GTEN_WAVE) void k_col_energy_partials(const uint8_t* __restrict__ x, size_t pitch, int n_rows, int n_cols,
                                                                   double* __restrict__ part)
{
    using F = EnergyFmt<DT>;
    constexpr int SLOTS = F::TILE_BYTES / 16 + 1;                   // 16-byte requests of one row's tile, misaligned at worst
    constexpr int NLOAD = (CE_STEP * SLOTS + GTEN_WAVE - 1) / GTEN_WAVE;
    __shared__ uint4 stage[CE_STEP * SLOTS];
    const int lane = threadIdx.x, chunk = blockIdx.x, col0 = blockIdx.y * CE_TILE;
    const int row0 = chunk * CE_CHUNK;
    const int nr = min(CE_CHUNK, n_rows - row0);
    const int cols = min(CE_TILE, n_cols - col0);
    const int tile_bytes = (int)F::col_byte(cols);
    const uint8_t* tile = x + F::col_byte(col0);

    uint4 v[NLOAD];
    auto request = [&](int r0) {                                    // rows r0 .. of the chunk -> v
#pragma unroll
        for (int i = 0; i < NLOAD; i++) {
            const int idx = lane + i * GTEN_WAVE, r = r0 + idx / SLOTS, s = idx % SLOTS;
            v[i] = uint4{0, 0, 0, 0};
            if (idx < CE_STEP * SLOTS && r < nr) {
                const uint8_t* a = tile + (size_t)(row0 + r) * pitch;
                const int shift = (int)((uintptr_t)a & 15);
                if (s * 16 < shift + tile_bytes) v[i] = *reinterpret_cast<const uint4*>(a - shift + s * 16);
            }
        }
    };
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    request(0);
    for (int r0 = 0; r0 < nr; r0 += CE_STEP) {
#pragma unroll
        for (int i = 0; i < NLOAD; i++)
            if (lane + i * GTEN_WAVE < CE_STEP * SLOTS) stage[lane + i * GTEN_WAVE] = v[i];
        __syncthreads();
        if (r0 + CE_STEP < nr) request(r0 + CE_STEP);
        if (4 * lane < cols) {
            const int rows = min(CE_STEP, nr - r0);
            for (int r = 0; r < rows; r++) {
                const int shift = (int)((uintptr_t)(tile + (size_t)(row0 + r0 + r) * pitch) & 15);
                float xv[4];
                F::load4(reinterpret_cast<const uint8_t*>(stage + r * SLOTS) + shift, 4 * lane, xv);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float sq = xv[i] * xv[i];
                    acc[i] += (double)sq;
                }
            }
        }
        __syncthreads();
    }
    if (4 * lane < cols) {                                          // (n_cols % 32 == 0: a lane's four columns exist together)
        double* o = part + (size_t)chunk * n_cols + col0 + 4 * lane;
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = acc[i];
    }
}

__global__ __launch_bounds__(CE_TILE) void k_col_energy_add(const double* __restrict__ part, int chunks, int n_cols, double* __restrict__ acc)
{
    const int c = blockIdx.x * CE_TILE + threadIdx.x;
    if (c >= n_cols) return;
    double s = acc[c];
    for (int j = 0; j < chunks; j++) s += part[(size_t)j * n_cols + c];
    acc[c] = s;
}

// the chunk sums: library-owned, grown on demand, one per stream (as the pooling kernels' scratch)
static int col_energy_scratch(size_t bytes, double** out)
{
    static double* bufs[2] = {nullptr, nullptr};
    static size_t caps[2] = {0, 0};
    double*& buf = bufs[gtr::stream_index() & 1];
    size_t& cap = caps[gtr::stream_index() & 1];
    if (bytes > cap) {
        if (buf) { GTR_CHECK(hipStreamSynchronize(gtr::stream())); GTR_CHECK(hipFree(buf)); }
        buf = nullptr; cap = 0;
        GTR_CHECK(hipMalloc((void**)&buf, bytes + bytes / 2));
        cap = bytes + bytes / 2;
    }
    *out = buf;
    return 0;
}

extern "C" int gten_hip_calib_col_energy(const void* rows, int adtype, int n_rows, int cols, long long pitch, double* acc)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(rows && acc, "calib_col_energy: null pointer");
    GTR_REQUIRE(adtype == GTEN_F16 || adtype == GTEN_Q8, "calib_col_energy: bad activation dtype %d", adtype);
    GTR_REQUIRE(cols >= 32 && cols % 32 == 0 && cols <= (1 << 20), "calib_col_energy: unsupported width %d", cols);
    GTR_REQUIRE(n_rows >= 1 && n_rows <= (1 << 22), "calib_col_energy: bad row count %d", n_rows);
    GTR_REQUIRE(pitch >= (long long)gten_hip_row_bytes(adtype, cols) && pitch % 2 == 0 && (uintptr_t)rows % 2 == 0, "calib_col_energy: bad pitch %lld or base", pitch);
    GTR_REQUIRE((uintptr_t)acc % 8 == 0, "calib_col_energy: the accumulator must be 8-byte aligned");
    const int chunks = (n_rows + CE_CHUNK - 1) / CE_CHUNK, tiles = (cols + CE_TILE - 1) / CE_TILE;
    double* part = nullptr;
    if (int rc = col_energy_scratch((size_t)chunks * cols * sizeof(double), &part)) return rc;
    const uint8_t* xb = (const uint8_t*)rows;
    if (adtype == GTEN_Q8)
        GTR_LAUNCH(KT_ELEMWISE, k_col_energy_partials<GTEN_Q8>, dim3(chunks, tiles), dim3(GTEN_WAVE), 0, xb, (size_t)pitch, n_rows, cols, part);
    else
        GTR_LAUNCH(KT_ELEMWISE, k_col_energy_partials<GTEN_F16>, dim3(chunks, tiles), dim3(GTEN_WAVE), 0, xb, (size_t)pitch, n_rows, cols, part);
    gtr::kv_watch_touch(acc, (size_t)cols * sizeof(double));
    GTR_LAUNCH(KT_ELEMWISE, k_col_energy_add, dim3(tiles), dim3(CE_TILE), 0, (const double*)part, chunks, cols, acc);
    return 0;
}
