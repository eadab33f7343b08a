// gten_decode_kvq4.h -- 4-bit head-major K / V shadows: the switch, the shadows' description, the rounding operator on row views and
// the read-back of a shadow (include/gten_hip_kvq4.h); included by gten_decode.hip, which owns the decoder, the
// shadows' layout (gten_decode_attn_hm.h) and the import / attention kernels (gten_decode_attn_hm_kernels.h).

// R (gten_kvq4_math.h) in place: one wave per two neighbouring blocks of a row, lane t = element t & 31 of block 2 x + (t >> 5) -- bytes
// and half-words only, so every view inside the row-view contract (base and pitch multiples of 2) takes this one form.  A row with an
// odd number of blocks: the upper half of its last wave looks at the last block again and stores nothing.
__global__ __launch_bounds__(64) void k_kv_round_q4(uint8_t* __restrict__ rows, int n_rows, int n_blocks, size_t pitch)
{
    const int t = threadIdx.x, b = 2 * (int)blockIdx.x + (t >> 5);
    const bool own = b < n_blocks;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        uint8_t* blk = rows + (size_t)r * pitch + (size_t)min(b, n_blocks - 1) * GTEN_Q8_BYTES;
        const uint16_t d = *(const uint16_t*)blk;
        const int q = (int8_t)blk[2 + (t & 31)];
        uint16_t d4;
        const int q4 = hmq4_round_lane(q, d, d4);               // (every lane's d and q have arrived before the first store below)
        if (own) {
            store_global<uint8_t>(blk + 2 + (t & 31), (uint8_t)(int8_t)q4);
            if ((t & 31) == 0) store_global<uint16_t>(blk, d4);
        }
    }
}

// a 4-bit shadow matrix of one (sequence, layer, K | V) back as dense Q8 rows: workgroup = (position, kv head), lane = element --
// through the layout's offset functions, the ones the import, the appends and (in registers) the attention kernel go by.
// (4-bit shadows only, on purpose: a further caller of the Q8 layout's hm_*_off functions changes the argument ranges the compiler
//  propagates into them, and with that the instruction order of k_kv_import_hm and k_dec_attn_hm -- seen with
//  tools/kernel_instruction_counts.py; the parent's kernels keep their instruction text.)
__global__ __launch_bounds__(64) void k_kv_shadow_read_q4(const uint8_t* __restrict__ sh, int n_chunks, int n_kv, int kv, uint8_t* __restrict__ out)
{
    const unsigned p = blockIdx.x, g = blockIdx.y, e = threadIdx.x, pp = p & (DEC_CHUNK - 1), blk = e >> 5;
    const uint8_t* c = sh + (size_t)(g * n_chunks + (p / DEC_CHUNK)) * HMQ4_CHUNK_BYTES;
    uint8_t* o = out + ((size_t)p * n_kv + g) * 68 + blk * GTEN_Q8_BYTES;
    const unsigned i = kv ? hmq4_v_q_off(pp, e) : hmq4_k_q_off(pp, e), doff = kv ? hmq4_v_d_off(pp, blk) : hmq4_k_d_off(pp, blk);
    const unsigned q = ((c[i >> 1] >> (4u * (i & 1u))) & 15u) - KVQ4_BIAS;
    o[2 + (e & 31u)] = (uint8_t)q;
    if ((e & 31u) == 0) *(uint16_t*)o = *(const uint16_t*)(c + doff);
}

extern "C" {

int gten_hip_set_kv_shadow_q4(int on)
{
    g_kv_shadow_q4 = on != 0;
    return 0;
}

int gten_hip_decoder_kv_shadow_info(gten_hip_decoder* dc, int* bits, int* chunk_bytes, unsigned long long* bytes_total)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_kv_shadow_info: null decoder");
    if (bits) *bits = !dc->hm ? 0 : dc->hm_q4 ? 4 : (dc->d.adtype == GTEN_Q8 || dc->hm_fp8) ? 8 : 16;
    if (chunk_bytes) *chunk_bytes = dc->hm ? (int)dc->hm_chunk_bytes : 0;
    if (bytes_total) *bytes_total = dc->hm ? (unsigned long long)dc->n_seq * dc->hm_seq_stride : 0ull;
    return 0;
}

int gten_hip_kv_round_q4(void* rows, int n_rows, size_t row_bytes, size_t pitch)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(rows && n_rows >= 1, "kv_round_q4: %d rows", n_rows);
    GTR_REQUIRE(row_bytes >= GTEN_Q8_BYTES && row_bytes % GTEN_Q8_BYTES == 0, "kv_round_q4: rows of %zu bytes are no whole Q8 blocks (34 bytes each)", row_bytes);
    GTR_REQUIRE(row_bytes / GTEN_Q8_BYTES <= (1u << 20), "kv_round_q4: rows of %zu bytes", row_bytes);
    GTR_REQUIRE((uintptr_t)rows % 2 == 0 && pitch % 2 == 0 && pitch >= row_bytes,
                "kv_round_q4: base %p and pitch %zu for rows of %zu bytes (multiples of 2, the pitch at least a row)", rows, pitch, row_bytes);
    const int n_blocks = (int)(row_bytes / GTEN_Q8_BYTES);
    GTR_LAUNCH(KT_PACK, k_kv_round_q4, dim3((unsigned)(n_blocks + 1) / 2, (unsigned)std::min(n_rows, 65535)), dim3(64), 0, (uint8_t*)rows, n_rows, n_blocks, pitch);
    // like every other writer of cache rows (the last row's pitch padding is not written, nor announced)
    kv_watch_touch(rows, (size_t)(n_rows - 1) * pitch + row_bytes);
    return 0;
}

int gten_hip_decoder_kv_shadow_read(gten_hip_decoder* dc, int seq, int layer, int kv, int n_rows, void* out_rows)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && out_rows, "decoder_kv_shadow_read: null argument");
    GTR_REQUIRE(dc->hm && dc->hm_q4, "decoder_kv_shadow_read: the decoder keeps no 4-bit shadows");
    GTR_REQUIRE(seq >= 0 && seq < dc->n_seq && layer >= 0 && layer < dc->d.n_layers && (kv == 0 || kv == 1),
                "decoder_kv_shadow_read: sequence %d, layer %d, matrix %d", seq, layer, kv);
    GTR_REQUIRE(n_rows >= 1 && n_rows <= dc->d.max_ctx, "decoder_kv_shadow_read: %d rows of a context of %d", n_rows, dc->d.max_ctx);
    const size_t bytes = (size_t)n_rows * dc->d.n_kv_heads * 68;
    uint8_t* dev = nullptr;
    GTR_CHECK(hipMalloc((void**)&dev, bytes));
    const uint8_t* sh = dc->hm + (size_t)seq * dc->hm_seq_stride + (size_t)(layer * 2 + kv) * dc->hm_cache_bytes;
    hipLaunchKernelGGL(k_kv_shadow_read_q4, dim3((unsigned)n_rows, (unsigned)dc->d.n_kv_heads), dim3(64), 0, stream(), sh, dc->n_chunks, dc->d.n_kv_heads,
                       kv, dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out_rows, dev, bytes, hipMemcpyDeviceToHost, stream());
    if (e == hipSuccess) e = hipStreamSynchronize(stream());
    (void)hipFree(dev);
    GTR_CHECK(e);
    return 0;
}

} // extern "C"
