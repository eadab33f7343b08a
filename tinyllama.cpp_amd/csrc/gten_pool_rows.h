// gten_pool_rows.h -- k_pool_partials and k_pool_finish, the kernels of gten_hip_pool_rows (include/gten_hip_embed.h, which
// states what they compute); included by gten_ops.hip.  DESIGN.md §3.22.
#pragma once

#include "gten_dev.h"
#include "gten_hip_embed.h"

// Both kernels fetch a row's bytes as ALIGNED 16-byte requests into LDS and take values apart there: a Q8 block is 34
// bytes, so a quant and its block's delta are only 2-byte aligned in a row, and a row itself starts wherever the pitch puts it.
// A request starts at the row's address rounded down to 16 and is issued only where it overlaps a byte that is needed, so
// it never leaves the 4 KB page of a byte the caller owns.
//
// Sums start from -0, the identity of IEEE addition (-0 + x == x for every x, -0 and +0 included): the result is the sum
// that starts from its first term, as the header defines it.
namespace {
constexpr int POOL_CHUNK = 64;        // rows of a chunk (the definition's)
constexpr int POOL_STEP = 16;         // rows staged in LDS at a time
constexpr int POOL_TILE = 256;        // columns of a workgroup of k_pool_partials: 4 per lane
constexpr int POOL_FIN_THREADS = 1024;   // k_pool_finish: at 2048 columns two per thread
constexpr int POOL_FIN_BATCH = 16;       // chunk sums requested together before they are added

// the host's segment table, passed by value (uniform reads of the kernel arguments, no device copy to keep alive)
struct PoolSegs {
    int32_t start[GTEN_HIP_POOL_MAX_SEGMENTS + 1];     // first row of segment k; [n] = the end of the last
    int32_t chunk0[GTEN_HIP_POOL_MAX_SEGMENTS + 1];    // chunks before segment k; [n] = all
    int32_t n;
};

template <int DT> struct PoolFmt;
template <> struct PoolFmt<GTEN_Q8> {
    static constexpr int TILE_BYTES = POOL_TILE / GTEN_QBLK * GTEN_Q8_BYTES;   // 272
    __device__ static size_t col_byte(int c) { return (size_t)(c / GTEN_QBLK) * GTEN_Q8_BYTES; }           // c % 32 == 0
    // columns c0 .. c0 + 3 (c0 % 4 == 0) of the bytes at p (2-byte aligned, column 0's block first)
    __device__ static void load4(const uint8_t* p, int c0, float* v)
    {
        const uint8_t* b = p + (c0 >> 5) * GTEN_Q8_BYTES;
        const float d = gtd::h2f(*reinterpret_cast<const uint16_t*>(b));
        const uint16_t* q = reinterpret_cast<const uint16_t*>(b + 2 + (c0 & 31));
        const uint16_t lo = q[0], hi = q[1];
        v[0] = (float)(int8_t)(lo & 0xff) * d;
        v[1] = (float)(int8_t)(lo >> 8) * d;
        v[2] = (float)(int8_t)(hi & 0xff) * d;
        v[3] = (float)(int8_t)(hi >> 8) * d;
    }
    __device__ static float load1(const uint8_t* p, int c)
    {
        const uint8_t* b = p + (c >> 5) * GTEN_Q8_BYTES;
        return (float)(int8_t)b[2 + (c & 31)] * gtd::h2f(*reinterpret_cast<const uint16_t*>(b));
    }
};
template <> struct PoolFmt<GTEN_F16> {
    static constexpr int TILE_BYTES = POOL_TILE * 2;                           // 512
    __device__ static size_t col_byte(int c) { return (size_t)c * 2; }
    __device__ static void load4(const uint8_t* p, int c0, float* v)
    {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p) + c0;
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = gtd::h2f(h[i]);
    }
    __device__ static float load1(const uint8_t* p, int c) { return gtd::h2f(reinterpret_cast<const uint16_t*>(p)[c]); }
};
} // namespace

// p_j of the header: one wave per (chunk, tile of POOL_TILE columns); lane l owns columns 4 l .. 4 l + 3 of the tile and adds
// the chunk's rows in ascending order.  POOL_STEP rows are staged at a time; the next step's requests are in flight while
// this step's rows are added.  part: f32 [all chunks][n_embd].
template <int DT>
__global__ __launch_bounds__(GTEN_WAVE) void k_pool_partials(const uint8_t* __restrict__ x, size_t pitch, int n_embd, PoolSegs segs,
                                                             float* __restrict__ part)
{
    using F = PoolFmt<DT>;
    constexpr int SLOTS = F::TILE_BYTES / 16 + 1;                   // 16-byte requests of one row's tile, misaligned at worst
    constexpr int NLOAD = (POOL_STEP * SLOTS + GTEN_WAVE - 1) / GTEN_WAVE;
    __shared__ uint4 stage[POOL_STEP * SLOTS];
    const int lane = threadIdx.x, chunk = blockIdx.x, col0 = blockIdx.y * POOL_TILE;
    int k = 0;
    while (k + 1 < segs.n && segs.chunk0[k + 1] <= chunk) k++;      // (uniform: at most 31 steps over kernel arguments)
    const int j = chunk - segs.chunk0[k];
    const int row0 = segs.start[k] + j * POOL_CHUNK;
    const int nr = min(POOL_CHUNK, segs.start[k + 1] - row0);
    const int cols = min(POOL_TILE, n_embd - col0);
    const int tile_bytes = (int)F::col_byte(cols);
    const uint8_t* tile = x + F::col_byte(col0);

    uint4 v[NLOAD];
    auto request = [&](int r0) {                                    // rows r0 .. of the chunk -> v
#pragma unroll
        for (int i = 0; i < NLOAD; i++) {
            const int idx = lane + i * GTEN_WAVE, r = r0 + idx / SLOTS, s = idx % SLOTS;
            v[i] = uint4{0, 0, 0, 0};
            if (idx < POOL_STEP * SLOTS && r < nr) {
                const uint8_t* a = tile + (size_t)(row0 + r) * pitch;
                const int shift = (int)((uintptr_t)a & 15);
                if (s * 16 < shift + tile_bytes) v[i] = *reinterpret_cast<const uint4*>(a - shift + s * 16);
            }
        }
    };
    float acc[4] = {-0.f, -0.f, -0.f, -0.f};
    request(0);
    for (int r0 = 0; r0 < nr; r0 += POOL_STEP) {
#pragma unroll
        for (int i = 0; i < NLOAD; i++)
            if (lane + i * GTEN_WAVE < POOL_STEP * SLOTS) stage[lane + i * GTEN_WAVE] = v[i];
        __syncthreads();
        if (r0 + POOL_STEP < nr) request(r0 + POOL_STEP);
        if (4 * lane < cols) {
            const int rows = min(POOL_STEP, nr - r0);
            for (int r = 0; r < rows; r++) {
                const int shift = (int)((uintptr_t)(tile + (size_t)(row0 + r0 + r) * pitch) & 15);
                float xv[4];
                F::load4(reinterpret_cast<const uint8_t*>(stage + r * SLOTS) + shift, 4 * lane, xv);
#pragma unroll
                for (int i = 0; i < 4; i++) acc[i] += xv[i];
            }
        }
        __syncthreads();
    }
    if (4 * lane < cols) {
        float4* o = reinterpret_cast<float4*>(part + (size_t)chunk * n_embd + col0 + 4 * lane);
        *o = float4{acc[0], acc[1], acc[2], acc[3]};
    }
}

// one workgroup of POOL_FIN_THREADS per segment: m (the chunk sums added in ascending j and divided by n, or the last row taken apart in LDS),
// then the normalisation.  Dynamic LDS: m as f32 [n_embd], behind it the staged row of last pooling.
template <int DT>
__global__ __launch_bounds__(POOL_FIN_THREADS) void k_pool_finish(const uint8_t* __restrict__ x, size_t pitch, int n_embd, PoolSegs segs,
                                                                  const float* __restrict__ part, int pooling, int normalize,
                                                                  float* __restrict__ out)
{
    using F = PoolFmt<DT>;
    extern __shared__ uint4 pool_lds[];
    __shared__ double t[GTEN_WAVE];
    float* m = reinterpret_cast<float*>(pool_lds);
    const int tid = threadIdx.x, k = blockIdx.x;
    const int n = segs.start[k + 1] - segs.start[k];
    if (pooling == GTEN_HIP_POOL_MEAN) {
        const int nc = segs.chunk0[k + 1] - segs.chunk0[k];
        const float* p = part + (size_t)segs.chunk0[k] * n_embd;
        for (int c = tid; c < n_embd; c += POOL_FIN_THREADS) {
            // a long text has up to 32 chunk sums per column: POOL_FIN_BATCH of them are requested before the first is added, so the
            // column waits for two round trips, not for one per chunk (a missing one counts as -0, which changes no sum)
            float s = -0.f;
            for (int j0 = 0; j0 < nc; j0 += POOL_FIN_BATCH) {
                float v[POOL_FIN_BATCH];
#pragma unroll
                for (int i = 0; i < POOL_FIN_BATCH; i++) v[i] = j0 + i < nc ? p[(size_t)(j0 + i) * n_embd + c] : -0.f;
#pragma unroll
                for (int i = 0; i < POOL_FIN_BATCH; i++) s += v[i];
            }
            m[c] = s / (float)n;
        }
    } else {
        uint4* stage = pool_lds + n_embd / 4;
        const uint8_t* a = x + (size_t)(segs.start[k + 1] - 1) * pitch;
        const int shift = (int)((uintptr_t)a & 15);
        const int slots = (shift + (int)F::col_byte(n_embd) + 15) / 16;
        for (int s = tid; s < slots; s += POOL_FIN_THREADS) stage[s] = *reinterpret_cast<const uint4*>(a - shift + s * 16);
        __syncthreads();
        for (int c = tid; c < n_embd; c += POOL_FIN_THREADS) m[c] = F::load1(reinterpret_cast<const uint8_t*>(stage) + shift, c);
    }
    __syncthreads();
    float* o = out + (size_t)k * n_embd;
    if (!normalize) {
        for (int c = tid; c < n_embd; c += POOL_FIN_THREADS) o[c] = m[c];
        return;
    }
    if (tid < GTEN_WAVE) {
        double s = 0.0;                                             // (every term is >= +0: 0 + the first term is the first term)
        for (int c = tid; c < n_embd; c += GTEN_WAVE) s += (double)m[c] * (double)m[c];
        t[tid] = s;
    }
    __syncthreads();
    double ss = t[0];
    for (int i = 1; i < GTEN_WAVE; i++) ss += t[i];
    const double root = sqrt(ss);
    for (int c = tid; c < n_embd; c += POOL_FIN_THREADS) o[c] = ss == 0.0 ? 0.f : (float)((double)m[c] / root);
}
