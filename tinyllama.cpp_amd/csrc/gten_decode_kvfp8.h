// gten_decode_kvfp8.h -- FP8 (E4M3) head-major K / V shadows of the f16 wide decoders: the switch, the rounding operator on row views
// and the read-back of a shadow (include/gten_hip_kvfp8.h); included by gten_decode.hip, which owns the decoder, the
// shadows' layout (gten_decode_attn_hm.h) and the import / attention kernels (gten_decode_attn_hm_kernels.h).

// R (gten_kvfp8_math.h) in place, one thread per element: half-words only, so every view inside the row-view contract (base and pitch
// multiples of 2) takes this one form.  R8 by the shared integer text, E8 by the instruction the attention kernel expands with.
__global__ __launch_bounds__(256) void k_kv_round_fp8(uint8_t* __restrict__ rows, int n_rows, unsigned n_halfs, size_t pitch)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= n_halfs) return;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        uint16_t* x = (uint16_t*)(rows + (size_t)r * pitch) + e;
        store_global<uint16_t>(x, (uint16_t)(hmf8_lo2(kvfp8_r8(*x)) & 0xffffu));
    }
}

// an FP8 shadow matrix of one (sequence, layer, K | V) back as dense f16 rows: workgroup = (position, kv head), lane = element -- through
// the layout's offset functions and the kernel's expansion
__global__ __launch_bounds__(64) void k_kv_shadow_read_fp8(const uint8_t* __restrict__ sh, int n_chunks, int n_kv, int kv, uint16_t* __restrict__ out)
{
    const unsigned p = blockIdx.x, g = blockIdx.y, e = threadIdx.x, pp = p & (DEC_CHUNK - 1);
    const uint8_t* c = sh + (size_t)(g * n_chunks + (p / DEC_CHUNK)) * HMF8_CHUNK_BYTES;
    out[((size_t)p * n_kv + g) * 64 + e] = (uint16_t)(hmf8_lo2(c[kv ? hmf8_v_off(pp, e) : hmf8_k_off(pp, e)]) & 0xffffu);
}

extern "C" {

int gten_hip_set_kv_shadow_fp8(int on)
{
    g_kv_shadow_fp8 = on != 0;
    return 0;
}

int gten_hip_kv_round_fp8(void* rows, int n_rows, size_t row_bytes, size_t pitch)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(rows && n_rows >= 1, "kv_round_fp8: %d rows", n_rows);
    GTR_REQUIRE(row_bytes >= 2 && row_bytes % 2 == 0 && row_bytes <= ((size_t)1 << 26), "kv_round_fp8: rows of %zu bytes are no whole f16 elements", row_bytes);
    GTR_REQUIRE((uintptr_t)rows % 2 == 0 && pitch % 2 == 0 && pitch >= row_bytes,
                "kv_round_fp8: base %p and pitch %zu for rows of %zu bytes (multiples of 2, the pitch at least a row)", rows, pitch, row_bytes);
    const unsigned n_halfs = (unsigned)(row_bytes / 2);
    GTR_LAUNCH(KT_PACK, k_kv_round_fp8, dim3((n_halfs + 255u) / 256u, (unsigned)std::min(n_rows, 65535)), dim3(256), 0, (uint8_t*)rows, n_rows, n_halfs, pitch);
    // like every other writer of cache rows (the last row's pitch padding is not written, nor announced)
    kv_watch_touch(rows, (size_t)(n_rows - 1) * pitch + row_bytes);
    return 0;
}

int gten_hip_decoder_kv_shadow_read_fp8(gten_hip_decoder* dc, int seq, int layer, int kv, int n_rows, void* out_rows)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && out_rows, "decoder_kv_shadow_read_fp8: null argument");
    GTR_REQUIRE(dc->hm && dc->hm_fp8, "decoder_kv_shadow_read_fp8: the decoder keeps no FP8 shadows");
    GTR_REQUIRE(seq >= 0 && seq < dc->n_seq && layer >= 0 && layer < dc->d.n_layers && (kv == 0 || kv == 1),
                "decoder_kv_shadow_read_fp8: sequence %d, layer %d, matrix %d", seq, layer, kv);
    GTR_REQUIRE(n_rows >= 1 && n_rows <= dc->d.max_ctx, "decoder_kv_shadow_read_fp8: %d rows of a context of %d", n_rows, dc->d.max_ctx);
    const size_t bytes = (size_t)n_rows * dc->d.n_kv_heads * 128;
    uint16_t* dev = nullptr;
    GTR_CHECK(hipMalloc((void**)&dev, bytes));
    const uint8_t* sh = dc->hm + (size_t)seq * dc->hm_seq_stride + (size_t)(layer * 2 + kv) * dc->hm_cache_bytes;
    hipLaunchKernelGGL(k_kv_shadow_read_fp8, dim3((unsigned)n_rows, (unsigned)dc->d.n_kv_heads), dim3(64), 0, stream(), sh, dc->n_chunks, dc->d.n_kv_heads,
                       kv, dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out_rows, dev, bytes, hipMemcpyDeviceToHost, stream());
    if (e == hipSuccess) e = hipStreamSynchronize(stream());
    (void)hipFree(dev);
    GTR_CHECK(e);
    return 0;
}

} // extern "C"
