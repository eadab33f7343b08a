// gten_decode_oplanes.h: the o projection of the single-sequence fast step as four K-quarter planes (k_dec_o_planes) -- part of the
// single-token decode translation unit: included by gten_decode.hip behind gten_decode_wx.h, whose building blocks it uses.
//
// k_dec_gemv8<.., PRO_ATTW, ..> makes EVERY one of its 256 workgroups request and join the chunk partials of all 32 heads (64 KB
// and the statistics) and stage the whole 2048-wide vector before it dots its eight rows: a 16.8 MB broadcast out of the L2s per
// launch, and the join and the staging 256 times over.  A row's dot is a sum over K, and wave_sum's tree (gten_dev.h) already
// splits K into four independent quarters: lane l holds block l of 64, quads / row_half_mirror / row_mirror leave in every lane of
// 16-lane row i the tree R_i over blocks 16 i .. 16 i + 15, and row_bcast15 (rows 1, 3) and row_bcast31 (rows 2, 3) put
// (R3 + R2) + (R1 + R0) into lane 63.  f32 addition is commutative, so the row is (p0 + p1) + (p2 + p3) with p_q the 16-lane tree
// over K quarter q, bit for bit (tests/test_o_planes_tree_cpu.py).
//
// A quarter is 16 blocks = 512 elements = heads 8 q .. 8 q + 7 at d_head 64.  One workgroup per (group of 32 rows, quarter q):
// it requests only its eight heads' statistics and partials (16 KB), joins and stages 512 elements -- one per thread, a Q8 block
// is a half wave -- and a wave dots four rows, a 16-lane row of the wave per weight row.  One lane per row stores p_q[row] into
// plane q of the output (OPL_PLANES x n_embd floats); the consumer (gate|up: k_dec_gemv8<.., NPL = OPL_PLANES>) adds the planes in
// the order above.  The join is PRO_ATTW's arithmetic and the staging q8_stageN's, element by element, so plane sums, residual
// rows and everything behind them keep the bytes of the one-plane launch (tests/test_decode_o_planes_gpu.py).
//
// Shape: n_embd 2048, d_head 64, Q8 activations, q4 or q8 weights (decoder_build selects it; everything else keeps k_dec_gemv8).

#define OPL_PLANES 4              // K quarters = output planes
#define OPL_E 2048                // n_embd this kernel is written for
#define OPL_LDS (OPL_E / OPL_PLANES + (OPL_E / OPL_PLANES / 32) * 8)       // the staged quarter: quants | deltas | sums

// the words (all preloadable): att_part | att_stats | quants of wo (its deltas follow them) | step | out | n_chunks
template <int WT, int WLD>
__global__ __launch_bounds__(512) void k_dec_o_planes(const unsigned long long h0, const unsigned long long h1, const unsigned long long h2,
                                                      const unsigned long long h3, const unsigned long long h4, const unsigned long long h5)
{
    static_assert(WT == GTEN_Q4 || WT == GTEN_Q8, "quantized weights (Q8 activations)");
    constexpr int NB = OPL_E / 32;                // blocks of a weight row
    constexpr int QB = NB / OPL_PLANES;           // ... of a quarter
    constexpr int WBYTES = (WT == GTEN_Q4) ? 16 : 32;
    static_assert(QB == 16 && OPL_E / OPL_PLANES == 512, "a quarter is one 16-lane row of blocks and one element per thread");
    const float* att_part = from_word<float>(h0);
    const float2* att_stats = from_word<float2>(h1);
    const uint8_t* qs = from_word<uint8_t>(h2);
    const DecStep* step = from_word<DecStep>(h3);
    const unsigned att_chunks = (unsigned)h5;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    // workgroups are dealt to the eight XCDs round robin: two neighbours in that deal share a quarter, so an L2 serves one
    // quarter's partials (speed only -- every workgroup computes from its own (group, quarter), wherever it runs)
    const unsigned q = (blockIdx.x & 7u) >> 1, grp = ((blockIdx.x >> 3) << 1) | (blockIdx.x & 1u);
    const int n = step[0].n;

    // ---- 1. the statistics and chunk partials of this thread's element: head 8 q + wid, element `lane` of it (stale chunks
    //         are readable and dropped by a select below; decoder_create: n_chunks <= DEC_ATT_MAXCH)
    const unsigned row0 = (q * 8u + (unsigned)wid) * att_chunks;
    float2 cst[DEC_ATT_MAXCH];
    float apart[DEC_ATT_MAXCH];
#pragma unroll
    for (int j = 0; j < DEC_ATT_MAXCH; j++) cst[j] = att_stats[row0 + min((unsigned)j, att_chunks - 1u)];
#pragma unroll
    for (int j = 0; j < DEC_ATT_MAXCH; j++) apart[j] = att_part[((row0 + min((unsigned)j, att_chunks - 1u)) << 6) + (unsigned)lane];

    // ---- 2. this wave's weights: rows 4 wid .. 4 wid + 3 of the group, lane = (row lane >> 4, block lane & 15 of the quarter)
    const unsigned r = grp * 32u + (unsigned)wid * 4u + ((unsigned)lane >> 4), blk = q * QB + ((unsigned)lane & 15u);
    const uint16_t* ds = (const uint16_t*)(qs + (size_t)OPL_E * NB * WBYTES);
    uint4 wq, wq1 = make_uint4(0, 0, 0, 0);
    if (WT == GTEN_Q4) {
        wq = ld_w16<WLD>((const uint4*)(qs + (size_t)r * NB * 16) + blk);
    } else {
        const uint4* q0 = (const uint4*)(qs + (size_t)r * NB * 32);
        wq = ld_w16<WLD>(q0 + blk);
        wq1 = ld_w16<WLD>(q0 + NB + blk);
    }
    const uint16_t wd = ld_w2<WLD>(ds + (size_t)r * NB + blk);
    __builtin_amdgcn_sched_barrier(0);            // keep every request above ahead of the join's arithmetic

    // ---- 3. the join (PRO_ATTW's arithmetic, gten_decode_wx.h) and the staging (q8_stageN's; the block is a half wave)
    const int nch = (n + DEC_CHUNK - 1) / DEC_CHUNK;
    float M = -INFINITY;
#pragma unroll
    for (int j = 0; j < DEC_ATT_MAXCH; j++) M = fmaxf(M, (j < nch) ? cst[j].x : -INFINITY);
    float w[DEC_ATT_MAXCH], L = 0.f;
#pragma unroll
    for (int j = 0; j < DEC_ATT_MAXCH; j++) {
        w[j] = (j < nch) ? cst[j].y * __expf(cst[j].x - M) : 0.f;
        L += w[j];
    }
    const float rL = recip_rn(L);
#pragma unroll
    for (int j = 0; j < DEC_ATT_MAXCH; j++) w[j] = (nch == 1) ? 1.0f : w[j] * rL;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < DEC_ATT_MAXCH; j++) v += (j < nch) ? w[j] * apart[j] : 0.f;
    const ActQ8 st = actq8_carve(g_smem, QB);
    {
        const Q8Scale s = q8_scale_from_absmax(max32(fmaxf(0.f, fabsf(v))));
        const int qv = q8_round(v, s.scale);
        const int sum = sum32_i(qv);
        st.q[threadIdx.x] = (int8_t)qv;
        if ((lane & 31) == 0) { st.d[threadIdx.x >> 5] = s.ddeq; st.sum[threadIdx.x >> 5] = sum; }
    }
    __syncthreads();

    // ---- 4. this lane's block of the quarter against its weight block; the 16-lane tree of wave_sum; one lane per row stores
    const int bl = lane & 15;
    int av[8];
    {
        const int4* ap = (const int4*)(st.q + bl * 32);
        const int4 a0 = ap[0], a1 = ap[1];
        av[0] = a0.x; av[1] = a0.y; av[2] = a0.z; av[3] = a0.w;
        av[4] = a1.x; av[5] = a1.y; av[6] = a1.z; av[7] = a1.w;
    }
    const float ad = st.d[bl];
    const int asum = st.sum[bl];
    const int isum = (WT == GTEN_Q4) ? dot_q8_q4_block(av, asum, wq) : dot_q8_q8_block(av, wq, wq1);
    float acc = 0.f;
    acc += (float)isum * (ad * h2f(wd));
    acc += dpp_mov<0xB1>(acc);
    acc += dpp_mov<0x4E>(acc);
    acc += dpp_mov<0x141>(acc);
    acc += dpp_mov<0x140>(acc);                   // every lane of the 16-lane row holds p_q[r]
    if (bl == 15) store_global<float>((void*)(uintptr_t)(h4 + ((unsigned long long)q * OPL_E + r) * 4ull), acc);
}
