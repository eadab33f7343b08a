// gten_decode_attn_w.h: k_dec_attn_one64w, the single-sequence d_head 64 attention launch with helper waves -- part of the
// single-token decode translation unit (included by gten_decode.hip after gten_decode_attn.h).
//
// ---- k_dec_attn_one64v's bytes from a workgroup of EIGHT waves in two roles (single sequence; Q8 and f16 activations)
//
// k_dec_attn_one64v runs one wave per SIMD, so every instruction on a wave's path costs a full issue slot of wall time, and
// about 216 of the instructions between its scores and its chunk maximum only widen V for p.V, two barriers later.  Here a
// second wave per SIMD carries everything the softmax chain does not need:
//   * waves 0-3 (the chain): thread c requests its K row at entry; wave 0 makes the q head vector (A -> RoPE -> A); scores
//     (with the new position's second pass), chunk maximum, expf, chunk sum, the probability rounded to the activation dtype
//     and staged as [cg][k], the p.V chains (e, cg) over cg, cg + 4, ... joined as ((g0 + g1) + g2) + g3, the stores of
//     att_part and stats -- k_dec_attn_one64v's arithmetic, term by term, from the same reduction trees;
//   * waves 4-7 (the helpers): thread 256 + c requests position c's V row at entry and widens it to f32 into
//     vf[c][ATT1V_VROW] -- (float)q * fp16(delta), zeros at and beyond n -- in three parts, one per chain segment up to the
//     barrier that publishes p, so that the chain never waits for a helper that got its row when the chain got its own.
//     In the workgroup that holds the new position waves 4 and 5 prepare the new k and v rows (what waves 1 and 2 of the
//     other kernels do): ki8 / kd stay in LDS for the new position's score, the designated writer workgroup appends both
//     rows to the caches, and the new position's row of vf is the new v row.
// Every barrier is executed by all eight waves at workgroup-uniform control flow, outside the role branches; the helpers
// only pass through the reductions' barriers (the partial words of waves 0-3 are read in the order of block_max_n<4> /
// block_sum_n<4>).  The LDS layout is k_dec_attn_one64v's.  att_part, stats and the appended cache rows are bit-identical
// to k_dec_attn_one64v's, hence to k_dec_attn_one64's.
// (the split of the widening, measured on the step: 8 | 4 | 4 groups 2119-2126 tok/s, 16 | 0 | 0 2112-2119, 4 | 6 | 6 2113-2117)
#ifndef ATT1W_SPLIT_A
#define ATT1W_SPLIT_A 8          // of a V row's 16 four-float groups: widened beside the scores ...
#endif
#ifndef ATT1W_SPLIT_B
#define ATT1W_SPLIT_B 12         // ... up to here beside exp and the chunk sum, the rest beside the probabilities
#endif
template <int ADT>
__global__ __launch_bounds__(512) void k_dec_attn_one64w(const unsigned long long h0, const unsigned long long h1, const unsigned long long h2,
                                                        const unsigned long long h3, const unsigned long long h4, const unsigned long long h5,
                                                        const unsigned long long h6, const AttnArgs a0)
{
    AttnArgs a = a0;
    a.qkv_raw = from_word<float>(h0); a.rope_now = from_word<float2>(h1); a.kcache = (uint8_t*)from_word<uint8_t>(h2);
    a.step = from_word<DecStep>(h3); a.kv_pitch = (size_t)(unsigned)(h4 & 0xffffffffull); a.max_ctx = (int)(h4 >> 32);
    a.n_embd = (int)(unsigned)(h5 & 0xffffffffull); a.n_heads = (int)((h5 >> 32) & 0xffu); a.n_kv = (int)((h5 >> 40) & 0xffu); a.grp_shift1 = (int)(h5 >> 48);
    a.vcache = (uint8_t*)from_word<uint8_t>(h6);
    constexpr int dh = 64, nblk = 2;
    constexpr int NW = (ADT == GTEN_Q8) ? 17 : 32;     // dwords per kv-head slice
    constexpr int VS = ATT1V_VROW, PS = ATT1V_PCOL;     // floats per V row / per p column group in LDS
    const int h = blockIdx.y, chunk = blockIdx.x, c0 = chunk * DEC_CHUNK;
    const int grp = a.grp_shift1 ? (1 << (a.grp_shift1 - 1)) : a.n_heads / a.n_kv, g = a.grp_shift1 ? (h >> (a.grp_shift1 - 1)) : h / grp;
    const int kv_dim = a.n_kv * dh;
    const size_t head_bytes = (ADT == GTEN_Q8) ? (size_t)nblk * GTEN_Q8_BYTES : (size_t)dh * 2;

    float* red = (float*)g_smem;                 // 16
    float* qf = red + 16 + dh;                   // dh
    float* kf = qf + dh;                         // dh
    float* qd = kf + dh;                         // 8
    float* kd = qd + 8;                          // 8
    uint16_t* d16 = (uint16_t*)(kd + 8);         // 16 halves
    int8_t* qi8 = (int8_t*)(d16 + 16);           // dh
    int8_t* ki8 = qi8 + dh;                      // dh
    int8_t* vi8 = ki8 + dh;                      // dh
    float* pt = (float*)(g_smem + 1152);         // 4 x PS: p of position cg + 4 k at pt[cg * PS + k]
    float* part = pt + 4 * PS;                   // 256
    float* vf = part + DEC_CHUNK;                // DEC_CHUNK x VS

    // ---- entry requests: the raw row this wave may turn into a head vector (wave 0: q, 4: k, 5: v) and its rotation, then
    //      this thread's cache row -- position lt's K row on the chain, its V row on the helpers
    const int pw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       // wave: 0-3 the chain, 4-7 the helpers
    const bool helper = pw >= 4;
    // (one static s_setprio 1 for the chain waves at entry measured SLOWER: 2082-2094 tok/s against 2119-2126, HISTORY.md)
    const int lt = threadIdx.x & 255, t = threadIdx.x & 63;
    const int c = c0 + lt;
    const int roff = (pw == 4) ? a.n_embd + g * dh : (pw >= 5) ? a.n_embd + kv_dim + g * dh : h * dh;
    const float raw = a.qkv_raw[roff + t];
    const float2 rot = a.rope_now[t & 31];
    __builtin_amdgcn_sched_barrier(0);
    const int cs = min(c, a.max_ctx - 1);
    const unsigned pitch_w = (unsigned)(a.kv_pitch >> 2);
    const gmem_u32 rp = as_global((helper ? a.vcache : a.kcache) + (size_t)g * head_bytes) + (unsigned)cs * pitch_w;
    unsigned rw[NW];
    {
        typedef unsigned u4u __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
        for (int j = 0; j + 4 <= NW; j += 4) {
            const u4u q = *(const __attribute__((address_space(1))) u4u*)(rp + j);
            rw[j] = q.x; rw[j + 1] = q.y; rw[j + 2] = q.z; rw[j + 3] = q.w;
        }
#pragma unroll
        for (int j = NW & ~3; j < NW; j++) rw[j] = rp[j];
    }
    __builtin_amdgcn_sched_barrier(0);
    const int n = a.step->n, pos = n - 1;
    if (c0 >= n) return;                                     // (all 512 threads)

    const bool has_new = (pos >= c0) && (pos < c0 + DEC_CHUNK);
    const bool writer = has_new && (h == g * grp);
    float vnew = 0.f;                             // wave 5: the new v row's element t (exact storage value)
    if (pw == 0 || (has_new && (pw == 4 || pw == 5))) {
        const int r = (pw == 0) ? 0 : pw - 3;     // 0: q, 1: the new k row, 2: the new v row
        int8_t* dq = (r == 0) ? qi8 : (r == 1) ? ki8 : vi8;
        float* dd = (r == 0) ? qd : (r == 1) ? kd : kd + 4;
        const float v = head_prep_cs(raw, true, r != 2, rot, dh, ADT, dq, dd, d16 + 4 * r);
        if (r == 0) qf[t] = v;
        if (r == 1) kf[t] = v;
        if (r == 2) vnew = v;
        if (r >= 1 && writer) {
            uint8_t* row = ((r == 1) ? a.kcache : a.vcache) + (size_t)pos * a.kv_pitch + (size_t)g * head_bytes;
            if (ADT == GTEN_Q8) {
                uint8_t* blk = row + (size_t)(t >> 5) * GTEN_Q8_BYTES;
                store_global<uint8_t>(blk + 2 + (t & 31), (uint8_t)dq[t]);
                if ((t & 31) == 0) store_global<uint16_t>(blk, d16[4 * r + (t >> 5)]);
            } else {
                store_global<uint16_t>((uint16_t*)row + t, f2h(v));
            }
        }
    }
    __syncthreads();                                         // q (and the new k row) for the chain

    // helpers: four-float groups [j0, j1) of this thread's V row as f32 into LDS (zeros at and beyond n; the new position's
    // row is the new v row, from wave 5)
    auto widen = [&](const int j0, const int j1) {
        if (c == pos) return;
        const bool live = c < n;
        float4* dst = (float4*)(vf + lt * VS);
#pragma unroll
        for (int j = j0; j < j1; j++) {
            float f[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int e = 4 * j + i;
                float x;
                if (ADT == GTEN_Q8) {
                    const int b = (e < 32) ? 2 + e : 4 + e;                  // byte of the 68-byte slice: [d0 | q0 x 32 | d1 | q1 x 32]
                    const int q = (int)(int8_t)(uint8_t)(rw[b >> 2] >> (8 * (b & 3)));
                    const float d = h2f((uint16_t)((e < 32) ? (rw[0] & 0xffffu) : (rw[8] >> 16)));
                    x = (float)q * d;
                } else {
                    x = h2f((uint16_t)((e & 1) ? (rw[e >> 1] >> 16) : (rw[e >> 1] & 0xffffu)));
                }
                f[i] = live ? x : 0.f;
            }
            dst[j] = make_float4(f[0], f[1], f[2], f[3]);
        }
    };

    float sc = -INFINITY, mx = 0.f, ex = 0.f, sm = 0.f;
    if (!helper) {
        // ---- scores (k_dec_attn_one64's arithmetic), then block_max_n<4>'s first half
        const float scale = 1.0f / sqrtf((float)dh);
        float acc = 0.f;
        if (ADT == GTEN_Q8) {
            const int* qi = (const int*)qi8;
            int isum = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) isum = dot4(qi[j], (int)__builtin_amdgcn_alignbit(rw[j + 1], rw[j], 16), isum);
            acc += (float)isum * (qd[0] * h2f((uint16_t)(rw[0] & 0xffffu)));
            isum = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) isum = dot4(qi[8 + j], (int)rw[9 + j], isum);
            acc += (float)isum * (qd[1] * h2f((uint16_t)(rw[8] >> 16)));
        } else {
#pragma unroll
            for (int j = 0; j < 32; j++) {
                acc += qf[2 * j] * h2f((uint16_t)(rw[j] & 0xffffu));
                acc += qf[2 * j + 1] * h2f((uint16_t)(rw[j] >> 16));
            }
        }
        if (has_new) {
            float accn = 0.f;
            if (ADT == GTEN_Q8) {
                const int* qi = (const int*)qi8;
                const int* ki = (const int*)ki8;
#pragma unroll
                for (int b = 0; b < nblk; b++) {
                    int isum = 0;
#pragma unroll
                    for (int j = 0; j < 8; j++) isum = dot4(qi[b * 8 + j], ki[b * 8 + j], isum);
                    accn += (float)isum * (qd[b] * kd[b]);
                }
            } else {
                for (int e = 0; e < dh; e++) accn += qf[e] * kf[e];
            }
            if (c == pos) acc = accn;
        }
        sc = (c < n) ? acc * scale : -INFINITY;
        const float wm = wave_max_dpp(sc);
        if (t == 0) red[pw] = wm;
    } else {
        widen(0, ATT1W_SPLIT_A);
    }
    __syncthreads();                                         // the chain waves' maxima
    if (!helper) {
        const float4 m4 = *(const float4*)red;
        mx = fmaxf(fmaxf(fmaxf(m4.x, m4.y), m4.z), m4.w);
        ex = (c < n) ? expf(sc - mx) : 0.f;
        const float ws = wave_sum(ex);
        if (t == 0) red[4 + pw] = ws;                       // (block_sum_n<4> on its own words)
    } else {
        widen(ATT1W_SPLIT_A, ATT1W_SPLIT_B);
    }
    __syncthreads();                                         // the chain waves' sums
    if (!helper) {
        const float4 s4 = *(const float4*)(red + 4);
        sm = 0.f;
        sm += s4.x; sm += s4.y; sm += s4.z; sm += s4.w;
        // ---- probabilities against the chunk's own statistics, rounded to the activation dtype in registers
        float pr = (c < n) ? ex / sm : 0.f;
        if (ADT == GTEN_Q8) {
            const Q8Scale s8 = q8_scale_from_absmax(max32(fabsf(pr)));
            if (c < n) pr = (float)q8_round(pr, s8.scale) * s8.ddeq;
        } else {
            pr = h2f(f2h(pr));
        }
        pt[(lt & 3) * PS + (lt >> 2)] = pr;
    } else {
        widen(ATT1W_SPLIT_B, 16);
        if (has_new && pw == 5) vf[(pos - c0) * VS + t] = vnew;
    }
    __syncthreads();                                         // p, and every V row

    // ---- p . V: chain (e, cg) over positions cg, cg + 4, ..., cg + 252 (waves 0-3)
    if (!helper) {
        const int e = t, cg = pw;
        const float* vcol = vf + cg * VS + e;
        const float4* pc = (const float4*)(pt + cg * PS);
        float o = 0.f;
#pragma unroll
        for (int j = 0; j < DEC_CHUNK / 16; j++) {
            const float4 p4 = pc[j];
            o = o + p4.x * vcol[(4 * j + 0) * 4 * VS];
            o = o + p4.y * vcol[(4 * j + 1) * 4 * VS];
            o = o + p4.z * vcol[(4 * j + 2) * 4 * VS];
            o = o + p4.w * vcol[(4 * j + 3) * 4 * VS];
        }
        part[lt] = o;
    }
    __syncthreads();
    if (threadIdx.x < dh) {
        float r = 0.f;
        for (int gi = 0; gi < 4; gi++) r += part[gi * dh + threadIdx.x];
        a.att_part[((size_t)h * a.n_chunks + chunk) * dh + threadIdx.x] = r;
    }
    if (threadIdx.x == 64) {
        a.stats[((size_t)h * a.n_chunks + chunk) * 2 + 0] = mx;
        a.stats[((size_t)h * a.n_chunks + chunk) * 2 + 1] = sm;
    }
}
