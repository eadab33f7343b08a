// gten_decode_attn_hm.h: decode attention of 16+ sequences on HEAD-MAJOR K / V shadows (round 5) -- part of the single-token
// decode translation unit: included by gten_decode.hip (which owns the includes, the LDS symbol, the launch macros and the
// host side).
//
// The reference keeps a K / V cache as rows [max_ctx][n_kv x 68 bytes] (gten/modules.cpp:188-201; a kv head's slice of a
// Q8 row = two 34-byte blocks, gten/quants.h:17-23), and so do the module tensors and every operator of this library.  A
// decode step of many sequences reads each cache once per step and little else: 92 % of the bytes of a 256-sequence step at
// ctx 2048.  A (kv head, 256-position chunk) workgroup reading 68-byte slices of 272-byte rows uses half of every
// 128-byte line it touches (round 4: 3.4-3.7 TB/s for the requests alone, against 5.1-5.5 TB/s for one contiguous run), and
// the slices then have to be re-laid in LDS before the matrix cores can take them.  A decoder of 16+ sequences (Q8
// activations, fast forms) therefore keeps a SHADOW of every sequence's caches, laid out for exactly this kernel:
//
//   shadow of one (sequence, layer, K | V):  [kv head][chunk of 256 positions][HM_CHUNK_BYTES = 17 408 = 256 x 68]
//   a K chunk   bytes [0, 16384)  the quants in MATRIX-OPERAND order: 16 tiles of 16 positions x 1 KiB; inside a tile lane
//               l = 16 lq + lc of a wave owns bytes [16 l, 16 l + 16) = elements 16 lq .. 16 lq + 15 of position 16 T + lc --
//               a tile is ONE coalesced 16-byte-per-lane load straight into the A operand of v_mfma_i32_16x16x64_i8
//               bytes [16384, 17408)  the block deltas (f16) as [block][lq][tile][4 positions]: a lane's 64 deltas are one
//               contiguous 128-byte run
//   a V chunk   bytes [0, 16384)  the quants TRANSPOSED and biased (q ^ 0x80), 8 steps of 32 positions x 2 KiB; lane l owns
//               16 bytes = two element tiles x 8 positions in the order the score tiles leave their probabilities in the
//               registers (slot j < 4: position 32 s + 4 lq + j, j >= 4: 32 s + 16 + 4 lq + j - 4): the A operand of
//               v_mfma_f32_16x16x32_f16 after a byte -> f16 expansion, no transpose through LDS
//               bytes [16384, 17408)  the block deltas as [lq][position pair][step][tile][position][half]: again one
//               128-byte run per lane
// The same 17 408 bytes per chunk as the cache rows hold, as ONE contiguous run per matrix.
//
// The row caches stay the truth: the shadows are filled from them (k_kv_import_hm) whenever a sequence (re)starts or
// anything wrote into its rows (gten_rt.h, kv_watch_*), the decode appends go to both, and every other path -- operators,
// the prompt kernels, decoders of up to 8 sequences, the exact forms, f16 activations -- reads the rows as before.
//
// k_dec_attn_hm: ONE WAVE per (sequence, kv head, chunk), no barrier against another wave, LDS only for the 8 head
// vectors of the group.  Scores as K . Q^T (positions on the rows): one v_mfma_i32_16x16x64_i8 per 16 positions gives, for
// the group's 8 heads, the exact integer dots of BOTH quant blocks at once -- columns 0..7 hold head j's block 0 (the B
// operand's lanes lq >= 2 are zero there), columns 8..15 head j's block 1 -- scaled (isum dq dk) and added across the
// column pair by one DPP rotate, exactly the two terms k_dec_attn_mm_g adds.  A lane then owns 2 of its tile's 4
// positions under one head: 32 scores per lane, every lane busy; maxima, sums of exponentials and the Q8 block maxima of
// the probabilities (32 positions along the context, gten/ops.h:996-997) are in-lane loops plus three cross-lane steps.
// The probabilities, rounded to Q8 and with the V row's block delta folded in (one fp16 rounding: k_dec_attn_mm_g's A
// operand), ARE the B operand of p.V as they stand (V^T x P^T, v_mfma_f32_16x16x32_f16): no LDS, no transpose.
// The new position never touches the chunk's registers: its score, probability and p.V term are formed from the chip's
// own K / V row beside the matrix instructions (its probability joins its Q8 block's maximum).
// Same chunk-local statistics and partials as k_dec_attn_mm_g (the consumer joins the chunks, PRO_ATTW); per (head,
// position) the same operations -- what differs is the order of the f32 additions in a chunk's sum of exponentials and in
// p.V (the matrix core's order over another assignment of positions to its steps).
// three waves per SIMD: the kernel fits 160 registers without a spill (hipcc takes 176 when left alone)
#ifndef HM_OCC
#define HM_OCC __attribute__((amdgpu_waves_per_eu(3)))
#endif
#define HM_CHUNK_BYTES 17408
#define HM_Q_BYTES 16384

// byte offsets inside a chunk: position p in [0, 256), element e in [0, 64), quant block / half in {0, 1}
__host__ __device__ __forceinline__ unsigned hm_k_q_off(unsigned p, unsigned e) { return (p >> 4) * 1024u + (((e >> 4) * 16u + (p & 15u)) * 16u) + (e & 15u); }
__host__ __device__ __forceinline__ unsigned hm_k_d_off(unsigned p, unsigned blk) { return HM_Q_BYTES + blk * 512u + ((p & 15u) >> 2) * 128u + (p >> 4) * 8u + (p & 3u) * 2u; }
__host__ __device__ __forceinline__ unsigned hm_v_q_off(unsigned p, unsigned e)
{
    const unsigned s = p >> 5, tp = (p >> 4) & 1u, r = p & 15u, et = e >> 4;
    return s * 2048u + (et >> 1) * 1024u + (((r >> 2) * 16u + (e & 15u)) * 16u) + (et & 1u) * 8u + 4u * tp + (r & 3u);
}
__host__ __device__ __forceinline__ unsigned hm_v_d_off(unsigned p, unsigned half)
{
    const unsigned s = p >> 5, tp = (p >> 4) & 1u, r = p & 15u;
    return HM_Q_BYTES + ((r >> 2) * 2u + ((r >> 1) & 1u)) * 128u + s * 16u + (tp * 4u + (r & 1u) * 2u + half) * 2u;
}

// ---- row caches -> shadows: one workgroup per (kv head, chunk) x (layer, K | V) x listed sequence.  Rows [0, n - 1) of a
// sequence at step n are its context (the step itself appends row n - 1); chunks without such a row return at once.
struct HmImportList { int n; int seq[512]; };

// ---- cross-lane steps of the one-wave kernel
__device__ __forceinline__ float hm_ror8(float v)               // the lane 8 columns away in its row of 16 (row_ror:8)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xF, 0xF, false));
}
__device__ __forceinline__ unsigned hm_ror8_u(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);
}
__device__ __forceinline__ float hm_rows_max(float v)           // over the four rows of 16 lanes (same column); every lane gets it
{
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float hm_rows_sum(float v)
{
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// four biased bytes (q ^ 0x80) -> four exact f16 integers: 0x6400 | b is 1024 + (q + 128); minus 1152
typedef _Float16 hm_h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void hm_bytes_to_h4(unsigned b4, unsigned& lo, unsigned& hi)
{
    const unsigned x0 = __builtin_amdgcn_perm(0x64646464u, b4, 0x04010400u);      // [b0, 0x64, b1, 0x64]
    const unsigned x1 = __builtin_amdgcn_perm(0x64646464u, b4, 0x04030402u);      // [b2, 0x64, b3, 0x64]
    const hm_h2 k = {(_Float16)1152.0f, (_Float16)1152.0f};
    lo = __builtin_bit_cast(unsigned, __builtin_bit_cast(hm_h2, x0) - k);
    hi = __builtin_bit_cast(unsigned, __builtin_bit_cast(hm_h2, x1) - k);
}

// Measured on the 256- / 64-sequence step (ms per step, two runs each, one box): waves per workgroup 4 | 2 and the
// K / V requests nontemporal or not -- 4: 3.145 3.155 / 1.506 1.514; 2: 3.201 3.192 / 1.501 1.497; 4 + nt: 3.136 3.106 / 1.539 1.538;
// 2 + nt: 3.105 3.110 / 1.516 1.511; one wave per workgroup (every wave prepares all eight head vectors) 3.153 / 1.515, two waves
// per SIMD instead of three 3.161 / 1.517.  So: pairs of chunks per workgroup, and the K / V stream -- read once per step, 6 GB
// at 256 sequences, far beyond the memory-side cache -- nontemporal from 128 rows per lane up (it then stops displacing the
// weights the other lane is about to read), default policy below.
// (Built and measured, round 5, not kept: ALL eight chunks of a (sequence, kv head) in one workgroup of eight waves, the partials and
//  statistics parked in LDS and joined on the chip with the consumer's arithmetic -- bit-identical logits, 1 MB of joined rows per
//  lane launch instead of 8.4 MB of partials written and read back -- 256 sequences 3.183 / 3.184 ms against 3.042 / 3.064 on the
//  same box, the launch 30.0 against 27.9 us; 64 sequences 1.500 against 1.488 ms.  One 512-thread workgroup per CU at 159 registers
//  runs its eight waves through request / softmax / p.V in lockstep and waits at the barrier for its slowest chunk, where six
//  independent pairs of waves per CU interleave those phases: the 17 MB per launch are cheaper than that.  HISTORY.md, round 5.)
#ifndef HM_WAVES
#define HM_WAVES 2            // waves per workgroup = consecutive chunks of one (sequence, kv head) that share the head vectors
#endif
#define HM_LD(p) (NT ? __builtin_nontemporal_load(p) : *(p))

// ---------------------------------------------------------------------------------------------------------------------------
// f16 activations (the f16 configuration's wide decoders; round 5).  The same idea with nothing to dequantize: a shadow chunk
// holds 256 positions x 64 halfs = 32 768 bytes per matrix, K as the A operands of v_mfma_f32_16x16x32_f16 (16 tiles x 2 steps
// of 32 elements: lane l owns the 8 halfs [16 l, 16 l + 16) of a (tile, step)), V TRANSPOSED as the A operands of the p.V
// products (8 steps of 32 positions x 4 element tiles; slot order as in the Q8 shadow).  One wave per (sequence, kv head, chunk):
// scores = K . Q^T (f16 products are exact in f32; the matrix core adds them), columns 0 .. GRP - 1 = the group's heads; a lane of
// a head column owns 4 positions per tile, so chunk maximum, sum of exponentials and the fp16 rounding of the probabilities
// (gten/ops.h:996-997 stores them as f16) are in-lane loops + two cross-lane steps, and the rounded probabilities are the B
// operand of p.V as they stand.  Chunk-local statistics, joined by the consumer (PRO_ATTW) -- the single-sequence f16 step's
// scheme instead of the row-global rounding of the two-launch pair this replaces.
#define HMF_CHUNK_BYTES 32768
__host__ __device__ __forceinline__ unsigned hmf_k_off(unsigned p, unsigned e)
{
    return (p >> 4) * 2048u + (e >> 5) * 1024u + (((((e & 31u) >> 3) * 16u) + (p & 15u)) * 16u) + (e & 7u) * 2u;
}
__host__ __device__ __forceinline__ unsigned hmf_v_off(unsigned p, unsigned e)
{
    return (p >> 5) * 4096u + (e >> 4) * 1024u + (((((p & 15u) >> 2) * 16u) + (e & 15u)) * 16u) + (4u * ((p >> 4) & 1u) + (p & 3u)) * 2u;
}

// A/B (GTEN_HIP_EXTRA_FLAGS=-DHM_PFX_SHARED_NT=1): the NT instantiations request SHARED chunks nontemporal too (DESIGN.md 3.9 has
// the measurement).  0: shared chunks always come with the default policy.
#ifndef HM_PFX_SHARED_NT
#define HM_PFX_SHARED_NT 0
#endif
// ---- the kernels: once as they always were, once with a shared prefix shadow beside the sequences' own (see the file)
#define HM_PFX 0
#define HM_KERNEL(name) name
#define HM_IMPORT_PFX_PARAMS
#define HM_ATTN_PFX_PARAMS
#include "gten_decode_attn_hm_kernels.h"
#undef HM_PFX
#undef HM_KERNEL
#undef HM_IMPORT_PFX_PARAMS
#undef HM_ATTN_PFX_PARAMS
#define HM_PFX 1
#define HM_KERNEL(name) name##_pfx
#define HM_IMPORT_PFX_PARAMS , const int* __restrict__ share
#define HM_ATTN_PFX_PARAMS , const uint8_t* __restrict__ pfx_k, const int* __restrict__ share
#include "gten_decode_attn_hm_kernels.h"
#undef HM_PFX
#undef HM_KERNEL
#undef HM_IMPORT_PFX_PARAMS
#undef HM_ATTN_PFX_PARAMS
// ... and once with a TABLE of prefix shadows (the attention kernels only; gten_hip_decoder_prefixes_set with an index above 0)
#define HM_PFX 2
#define HM_KERNEL(name) name##_pfxn
#define HM_ATTN_PFX_PARAMS , const uint8_t* const* __restrict__ pfx_tab, const size_t pfx_layer, const int* __restrict__ share, const int* __restrict__ which
#include "gten_decode_attn_hm_kernels.h"
#undef HM_PFX
#undef HM_KERNEL
#undef HM_ATTN_PFX_PARAMS

// the per-sequence shared counts and prefix indices (gten_hip_decoder_slot_share, gten_hip_decoder_prefixes_share): entry =
// sequence | chunks << 10 | prefix index << 16, written on the stream ahead of the imports and the steps that read them
struct HmShareList { int n; unsigned item[256]; };
__global__ __launch_bounds__(64) void k_hm_share_set(const HmShareList items, int* __restrict__ share, int* __restrict__ which)
{
    for (int i = threadIdx.x; i < items.n; i += 64) {
        const unsigned e = items.item[i];
        share[e & 1023u] = (int)((e >> 10) & 63u);
        which[e & 1023u] = (int)(e >> 16);
    }
}
