// gten_decode_sampler_api.h -- the sampler's entry points: top-k sampling (include/gten_hip_sample.h), bias tables
// (include/gten_hip_bias.h), log-probs of the generated ids (include/gten_hip_logprobs.h, §3.11) and top-p / min-p
// cuts (include/gten_hip_nucleus.h, §3.12) and penalties on repeated ids (include/gten_hip_penalty.h, §3.14).  Host code only; included
// by gten_decode.hip inside its extern "C" block, behind the decoder's other entry points.  The kernels are in gten_decode_sample.h,
// gten_decode_logprobs.h, gten_decode_nucleus.h and gten_decode_penalty.h; what
// the decoder keeps of a request, and which launch a step ends in, is SamplerState's comment in gten_decode.hip.

// ---- what the setters share
static int sample_check(int top_k, float temp, const char* who)
{
    GTR_REQUIRE(top_k >= 0, "%s: top_k %d < 0", who, top_k);
    GTR_REQUIRE(top_k == 0 || (std::isfinite(temp) && temp > 0.f), "%s: temperature %g must be finite and > 0 when top_k >= 1", who, (double)temp);
    return 0;
}
static int cut_check(float top_p, float min_p, const char* who)
{
    GTR_REQUIRE(std::isfinite(top_p) && top_p > 0.f && top_p <= 1.f, "%s: top_p %g outside (0, 1]", who, (double)top_p);
    GTR_REQUIRE(std::isfinite(min_p) && min_p >= 0.f && min_p <= 1.f, "%s: min_p %g outside [0, 1]", who, (double)min_p);
    return 0;
}
static CutParam cut_param(float top_p, float min_p)
{
    return CutParam{top_p, min_p > 0.f ? (float)std::log((double)min_p) : -INFINITY, min_p, (top_p == 1.f && min_p == 0.f) ? 0u : 1u};
}
static int pen_check(float r, float freq, float pres, const char* who)
{
    GTR_REQUIRE(std::isfinite(r) && r >= GTEN_HIP_PENALTY_R_MIN && r <= GTEN_HIP_PENALTY_R_MAX, "%s: repetition penalty %g outside [1/8, 8]", who, (double)r);
    GTR_REQUIRE(std::isfinite(freq) && std::fabs(freq) <= GTEN_HIP_PENALTY_ADD_MAX, "%s: frequency penalty %g (finite, |.| <= 100)", who, (double)freq);
    GTR_REQUIRE(std::isfinite(pres) && std::fabs(pres) <= GTEN_HIP_PENALTY_ADD_MAX, "%s: presence penalty %g (finite, |.| <= 100)", who, (double)pres);
    return 0;
}
static PenParam pen_param(float r, float freq, float pres, int start, int last_n)
{
    const bool off = r == 1.f && freq == 0.f && pres == 0.f;
    return PenParam{r, freq, pres, off ? 0 : start, off ? 0 : last_n, off ? 0u : 1u, {0u, 0u}};
}
// the counts of one row of n_vocab ids beside `kernel`'s own LDS: refused where they do not fit the CU's 160 KiB; otherwise the kernel's
// dynamic LDS limit is raised to them (outside any capture) and *lds is their size
#define PEN_LDS_CU (160 * 1024)
static int pen_fit(const void* kernel, int n_vocab, const char* who, size_t* lds)
{
    hipFuncAttributes fa;
    GTR_CHECK(hipFuncGetAttributes(&fa, kernel));
    const size_t need = pen_lds_bytes(n_vocab);
    GTR_REQUIRE(fa.sharedSizeBytes + need <= (size_t)PEN_LDS_CU, "%s: the counts of %d ids (%zu bytes) do not fit the workgroup's LDS beside the sampler's %zu",
                who, n_vocab, need, (size_t)fa.sharedSizeBytes);
    GTR_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
    *lds = need;
    return 0;
}

// sequence `seq`'s request as the host holds it, to the device (the steps queued before it have finished when this returns)
static int request_upload(gten_hip_decoder* dc, int seq)
{
    GTR_CHECK(hipMemcpyAsync(dc->smp.samp + seq, &dc->smp.samp_host[(size_t)seq], sizeof(SampleParam), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    return 0;
}

// The first use of a feature on this decoder (`on` is its SamplerState flag): with nothing in flight, `make` allocates and
// initialises what the feature needs (a buffer that an earlier call already made is kept); then the graphs captured so far are
// dropped -- they end in the rung below -- and from now on launch_step_end takes the feature's rung.
static int first_use(gten_hip_decoder* dc, bool& on, int (*make)(gten_hip_decoder*))
{
    GTR_CHECK(hipStreamSynchronize(stream()));
    if (int rc = make(dc)) return rc;
    GTR_CHECK(hipStreamSynchronize(stream()));
    GTR_CHECK(drop_graphs(dc));
    on = true;
    return 0;
}
static int bias_make(gten_hip_decoder* dc)          // every table: no bias
{
    if (dc->smp.bias) return 0;
    const size_t bytes = (size_t)GTEN_HIP_BIAS_TABLES * (size_t)dc->d.n_vocab * sizeof(float);
    GTR_CHECK(hipMalloc((void**)&dc->smp.bias, bytes));
    GTR_CHECK(hipMemsetAsync(dc->smp.bias, 0, bytes, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    return 0;
}
static int lp_make(gten_hip_decoder* dc)            // every record zeroed
{
    if (dc->smp.lp) return 0;
    const size_t bytes = (size_t)dc->n_seq * (size_t)(dc->d.max_ctx + 2) * sizeof(LpRecord);
    GTR_CHECK(hipMalloc((void**)&dc->smp.lp, bytes));
    GTR_CHECK(hipMemsetAsync(dc->smp.lp, 0, bytes, stream()));
    return 0;
}
static int cut_make(gten_hip_decoder* dc)           // every sequence: no cut
{
    SamplerState& s = dc->smp;
    s.cut_host.assign((size_t)dc->n_seq, cut_param(1.f, 0.f));
    if (!s.cut) GTR_CHECK(hipMalloc((void**)&s.cut, (size_t)dc->n_seq * sizeof(CutParam)));
    GTR_CHECK(hipMemcpyAsync(s.cut, s.cut_host.data(), s.cut_host.size() * sizeof(CutParam), hipMemcpyHostToDevice, stream()));
    return 0;
}
static int pen_make(gten_hip_decoder* dc)           // every sequence: no penalty; the kernel's LDS limit raised before any capture
{
    SamplerState& s = dc->smp;
    if (int rc = pen_fit((const void*)k_dec_sample_pen, dc->d.n_vocab, "decoder_set_penalty", &s.pen_lds)) return rc;
    s.pen_host.assign((size_t)dc->n_seq, pen_param(1.f, 0.f, 0.f, 0, 0));
    if (!s.pen) GTR_CHECK(hipMalloc((void**)&s.pen, (size_t)dc->n_seq * sizeof(PenParam)));
    GTR_CHECK(hipMemcpyAsync(s.pen, s.pen_host.data(), s.pen_host.size() * sizeof(PenParam), hipMemcpyHostToDevice, stream()));
    return 0;
}

// ---- the decoder's requests
int gten_hip_decoder_set_sampling(gten_hip_decoder* dc, int seq, int top_k, float temp, uint64_t seed, uint32_t stream_id)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && seq >= 0 && seq < dc->n_seq, "decoder_set_sampling: sequence %d outside [0, %d)", seq, dc ? dc->n_seq : 0);
    if (int rc = sample_check(top_k, temp, "decoder_set_sampling")) return rc;
    GTR_REQUIRE(top_k == 0 || !dc->persist_on, "decoder_set_sampling: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    SampleParam& p = dc->smp.samp_host[(size_t)seq];
    dc->smp.n_sampling += (top_k > 0 ? 1 : 0) - (p.top_k > 0 ? 1 : 0);
    p.top_k = top_k;
    p.temp = top_k > 0 ? temp : 0.f;
    p.stream = stream_id;
    p.seed_lo = (unsigned)(seed & 0xffffffffu);
    p.seed_hi = (unsigned)(seed >> 32);
    return request_upload(dc, seq);
}

int gten_hip_decoder_set_bias_table(gten_hip_decoder* dc, int table, const int32_t* ids_host, const float* values_host, int n, float fill)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_set_bias_table: null decoder");
    GTR_REQUIRE(!dc->persist_on, "decoder_set_bias_table: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    GTR_REQUIRE(table >= 0 && table < GTEN_HIP_BIAS_TABLES, "decoder_set_bias_table: table %d outside [0, %d)", table, GTEN_HIP_BIAS_TABLES);
    GTR_REQUIRE(n >= 0 && (n == 0 || (ids_host && values_host)), "decoder_set_bias_table: %d pairs, null lists", n);
    const int V = dc->d.n_vocab;
    auto value_ok = [](float v) { return v == -INFINITY || (std::isfinite(v) && std::fabs(v) <= GTEN_HIP_BIAS_MAX); };
    GTR_REQUIRE(value_ok(fill), "decoder_set_bias_table: fill %g (finite with |b| <= 1e30, or -inf)", (double)fill);
    std::vector<float> row((size_t)V, fill);
    std::vector<char> seen((size_t)V, 0);
    for (int i = 0; i < n; i++) {
        const int id = ids_host[i];
        GTR_REQUIRE(id >= 0 && id < V, "decoder_set_bias_table: id %d outside [0, %d)", id, V);
        GTR_REQUIRE(!seen[(size_t)id], "decoder_set_bias_table: id %d is listed twice", id);
        GTR_REQUIRE(value_ok(values_host[i]), "decoder_set_bias_table: value %g of id %d (finite with |b| <= 1e30, or -inf)", (double)values_host[i], id);
        seen[(size_t)id] = 1;
        row[(size_t)id] = values_host[i];
    }
    bool any = false;
    for (int j = 0; j < V && !any; j++) any = row[(size_t)j] > -INFINITY;
    GTR_REQUIRE(any, "decoder_set_bias_table: table %d would ban every id", table);
    if (int rc = bias_make(dc)) return rc;
    GTR_CHECK(hipMemcpyAsync(dc->smp.bias + (size_t)table * (size_t)V, row.data(), row.size() * sizeof(float), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));    // `row` lives on this stack frame
    return 0;
}

int gten_hip_decoder_set_seq_bias(gten_hip_decoder* dc, int seq, int table, int until)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && seq >= 0 && seq < dc->n_seq, "decoder_set_seq_bias: sequence %d outside [0, %d)", seq, dc ? dc->n_seq : 0);
    GTR_REQUIRE(table >= -1 && table < GTEN_HIP_BIAS_TABLES, "decoder_set_seq_bias: table %d outside [-1, %d)", table, GTEN_HIP_BIAS_TABLES);
    GTR_REQUIRE(until >= 0, "decoder_set_seq_bias: until %d < 0", until);
    GTR_REQUIRE(table < 0 || !dc->persist_on, "decoder_set_seq_bias: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    GTR_REQUIRE(table < 0 || !dc->smp.fsm_on || dc->smp.fsm_host[(size_t)seq].on == 0u,
                "decoder_set_seq_bias: sequence %d is bound to an automaton (gten_hip_decoder_set_seq_fsm): a table and an automaton do not compose", seq);
    if (table >= 0 && !dc->smp.bias_on)
        if (int rc = first_use(dc, dc->smp.bias_on, bias_make)) return rc;
    SampleParam& p = dc->smp.samp_host[(size_t)seq];
    dc->smp.n_bound += (table >= 0 ? 1 : 0) - (p.table1 > 0 ? 1 : 0);
    p.table1 = table + 1;
    p.until = table >= 0 ? (unsigned)until : 0u;
    return request_upload(dc, seq);
}

int gten_hip_decoder_bias_info(gten_hip_decoder* dc, int* n_tables, int32_t* table_host, int32_t* until_host, int table, const float** table_row)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_bias_info: null decoder");
    if (n_tables) *n_tables = GTEN_HIP_BIAS_TABLES;
    for (int q = 0; q < dc->n_seq; q++) {
        const SampleParam& p = dc->smp.samp_host[(size_t)q];
        if (table_host) table_host[q] = p.table1 - 1;
        if (until_host) until_host[q] = p.table1 > 0 ? (int32_t)p.until : 0;
    }
    if (table_row)
        *table_row = (dc->smp.bias && table >= 0 && table < GTEN_HIP_BIAS_TABLES) ? dc->smp.bias + (size_t)table * (size_t)dc->d.n_vocab : nullptr;
    return 0;
}

int gten_hip_decoder_set_logprobs(gten_hip_decoder* dc, int seq, int n_top)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && seq >= 0 && seq < dc->n_seq, "decoder_set_logprobs: sequence %d outside [0, %d)", seq, dc ? dc->n_seq : 0);
    GTR_REQUIRE(n_top >= -1 && n_top <= GTEN_HIP_LOGPROBS_TOP, "decoder_set_logprobs: n_top %d outside [-1, %d]", n_top, GTEN_HIP_LOGPROBS_TOP);
    GTR_REQUIRE(n_top < 0 || !dc->persist_on, "decoder_set_logprobs: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    if (n_top >= 0 && !dc->smp.lp_on)
        if (int rc = first_use(dc, dc->smp.lp_on, lp_make)) return rc;
    SampleParam& p = dc->smp.samp_host[(size_t)seq];
    dc->smp.n_asking += (n_top >= 0 ? 1 : 0) - (p.lp1 > 0u ? 1 : 0);
    p.lp1 = (unsigned)(n_top + 1);
    return request_upload(dc, seq);
}

int gten_hip_decoder_logprobs(gten_hip_decoder* dc, int seq, int n_from, int count, int n_top, float* logprob_host, int32_t* top_id_host,
                              float* top_logprob_host)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && seq >= 0 && seq < dc->n_seq, "decoder_logprobs: sequence %d outside [0, %d)", seq, dc ? dc->n_seq : 0);
    GTR_REQUIRE(n_top >= 0 && n_top <= GTEN_HIP_LOGPROBS_TOP, "decoder_logprobs: n_top %d outside [0, %d]", n_top, GTEN_HIP_LOGPROBS_TOP);
    GTR_REQUIRE(count >= 0 && n_from >= 0 && n_from + count <= dc->d.max_ctx + 2, "decoder_logprobs: positions [%d, %d + %d) outside [0, %d)", n_from, n_from,
                count, dc->d.max_ctx + 2);
    GTR_REQUIRE(dc->smp.lp, "decoder_logprobs: no sequence of this decoder has asked for log-probs (gten_hip_decoder_set_logprobs)");
    if (count == 0) return 0;
    GTR_REQUIRE(logprob_host && (n_top == 0 || (top_id_host && top_logprob_host)), "decoder_logprobs: null output");
    std::vector<LpRecord> rec((size_t)count);
    GTR_CHECK(hipMemcpyAsync(rec.data(), dc->smp.lp + (size_t)seq * (size_t)(dc->d.max_ctx + 2) + n_from, rec.size() * sizeof(LpRecord), hipMemcpyDeviceToHost,
                             stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    for (int i = 0; i < count; i++) {
        logprob_host[i] = rec[(size_t)i].logprob;
        for (int j = 0; j < n_top; j++) {
            top_id_host[(size_t)i * n_top + j] = rec[(size_t)i].top_id[j];
            top_logprob_host[(size_t)i * n_top + j] = rec[(size_t)i].top_logprob[j];
        }
    }
    return persist_aborted(dc);
}

int gten_hip_decoder_logprobs_info(gten_hip_decoder* dc, int* top_cap, int32_t* n_top_host, const void** records, long long* seq_stride_bytes,
                                   int* record_bytes)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_logprobs_info: null decoder");
    if (top_cap) *top_cap = GTEN_HIP_LOGPROBS_TOP;
    if (n_top_host) for (int q = 0; q < dc->n_seq; q++) n_top_host[q] = (int32_t)dc->smp.samp_host[(size_t)q].lp1 - 1;
    if (records) *records = dc->smp.lp;
    if (seq_stride_bytes) *seq_stride_bytes = (long long)(dc->d.max_ctx + 2) * (long long)sizeof(LpRecord);
    if (record_bytes) *record_bytes = (int)sizeof(LpRecord);
    return 0;
}

int gten_hip_decoder_set_cut(gten_hip_decoder* dc, int seq, float top_p, float min_p)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && seq >= 0 && seq < dc->n_seq, "decoder_set_cut: sequence %d outside [0, %d)", seq, dc ? dc->n_seq : 0);
    if (int rc = cut_check(top_p, min_p, "decoder_set_cut")) return rc;
    const CutParam c = cut_param(top_p, min_p);
    GTR_REQUIRE(c.on == 0u || !dc->persist_on, "decoder_set_cut: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    GTR_REQUIRE(c.on == 0u || !dc->smp.miro_on || dc->smp.miro_host[(size_t)seq].on == 0u,
                "decoder_set_cut: sequence %d is bound to mirostat (gten_hip_decoder_set_seq_mirostat): a cut and mirostat do not compose", seq);
    if (c.on == 0u && !dc->smp.cut_on) return 0;       // nobody has ever cut: nothing to clear
    if (!dc->smp.cut_on)
        if (int rc = first_use(dc, dc->smp.cut_on, cut_make)) return rc;
    dc->smp.cut_host[(size_t)seq] = c;
    GTR_CHECK(hipMemcpyAsync(dc->smp.cut + seq, &dc->smp.cut_host[(size_t)seq], sizeof(CutParam), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    return 0;
}

int gten_hip_decoder_cut_info(gten_hip_decoder* dc, float* top_p_host, float* min_p_host, float* t_host, int* on)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_cut_info: null decoder");
    for (int q = 0; q < dc->n_seq; q++) {
        const CutParam c = dc->smp.cut_on ? dc->smp.cut_host[(size_t)q] : cut_param(1.f, 0.f);
        if (top_p_host) top_p_host[q] = c.top_p;
        if (min_p_host) min_p_host[q] = c.min_p;
        if (t_host) t_host[q] = c.t;
    }
    if (on) *on = dc->smp.cut_on ? 1 : 0;
    return 0;
}

int gten_hip_decoder_set_penalty(gten_hip_decoder* dc, int seq, float r, float freq, float pres, int start, int last_n)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && seq >= 0 && seq < dc->n_seq, "decoder_set_penalty: sequence %d outside [0, %d)", seq, dc ? dc->n_seq : 0);
    if (int rc = pen_check(r, freq, pres, "decoder_set_penalty")) return rc;
    GTR_REQUIRE(start >= 0 && last_n >= 0, "decoder_set_penalty: window start %d, last_n %d (both >= 0)", start, last_n);
    const PenParam p = pen_param(r, freq, pres, start, last_n);
    GTR_REQUIRE(p.on == 0u || !dc->persist_on, "decoder_set_penalty: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    GTR_REQUIRE(p.on == 0u || dc->d.max_ctx < GTEN_HIP_PENALTY_HISTORY_MAX, "decoder_set_penalty: max_ctx %d >= %d (a count is 16 bits)", dc->d.max_ctx,
                GTEN_HIP_PENALTY_HISTORY_MAX);
    if (p.on == 0u && !dc->smp.pen_on) return 0;       // nobody has ever penalised: nothing to clear
    if (!dc->smp.pen_on)
        if (int rc = first_use(dc, dc->smp.pen_on, pen_make)) return rc;
    PenParam& h = dc->smp.pen_host[(size_t)seq];
    dc->smp.n_penalised += (p.on ? 1 : 0) - (h.on ? 1 : 0);
    h = p;
    GTR_CHECK(hipMemcpyAsync(dc->smp.pen + seq, &h, sizeof(PenParam), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    return 0;
}

int gten_hip_decoder_penalty_info(gten_hip_decoder* dc, float* r_host, float* freq_host, float* pres_host, int32_t* start_host, int32_t* last_n_host,
                                  int* on)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_penalty_info: null decoder");
    for (int q = 0; q < dc->n_seq; q++) {
        const PenParam p = dc->smp.pen_on ? dc->smp.pen_host[(size_t)q] : pen_param(1.f, 0.f, 0.f, 0, 0);
        if (r_host) r_host[q] = p.r;
        if (freq_host) freq_host[q] = p.freq;
        if (pres_host) pres_host[q] = p.pres;
        if (start_host) start_host[q] = p.start;
        if (last_n_host) last_n_host[q] = p.last_n;
    }
    if (on) *on = dc->smp.pen_on ? 1 : 0;
    return 0;
}

// ---- the row operators: the sampler on rows of logits that are not a decoder's
struct GrowBuf { void* dev = nullptr; size_t bytes = 0; };      // a device buffer that only grows
static GrowBuf g_rows_dev, g_cut_dev;                           // the per-row requests and cuts of one operator call
static GrowBuf g_pen_dev, g_hist_dev, g_off_dev;                // ... and their penalties, windows and window offsets

// what the penalty operators add to a call: every row's window and penalty; y_out: write the rows out instead of drawing from them
struct PenRows {
    const int32_t *hist, *off;
    const float *r, *freq, *pres;
    float* y_out;
    long long y_stride;
};

// `bytes` of the host's to the device buffer (grown when needed), queued on the stream
static int grow_upload(GrowBuf& b, const void* host, size_t bytes)
{
    if (b.bytes < bytes) {
        GTR_CHECK(hipStreamSynchronize(stream()));
        if (b.dev) GTR_CHECK(hipFree(b.dev));
        b = GrowBuf{};
        GTR_CHECK(hipMalloc(&b.dev, bytes));
        b.bytes = bytes;
    }
    GTR_CHECK(hipMemcpyAsync(b.dev, host, bytes, hipMemcpyHostToDevice, stream()));
    return 0;
}

// every row's window and penalty of a penalty operator, checked and uploaded (g_pen_dev, g_hist_dev, g_off_dev)
static int pen_rows_upload(const char* who, const PenRows& pen, int n_rows)
{
    GTR_REQUIRE(pen.off && pen.r && pen.freq && pen.pres, "%s: null argument", who);
    GTR_REQUIRE(pen.off[0] == 0, "%s: the first window offset is %d, not 0", who, pen.off[0]);
    std::vector<PenParam> pens((size_t)n_rows);
    for (int r = 0; r < n_rows; r++) {
        if (int rc = pen_check(pen.r[r], pen.freq[r], pen.pres[r], who)) return rc;
        const long long len = (long long)pen.off[r + 1] - (long long)pen.off[r];
        GTR_REQUIRE(len >= 0 && len <= GTEN_HIP_PENALTY_HISTORY_MAX, "%s: window of row %d has %lld ids (0 .. %d)", who, r, len, GTEN_HIP_PENALTY_HISTORY_MAX);
        pens[(size_t)r] = pen_param(pen.r[r], pen.freq[r], pen.pres[r], 0, 0);
    }
    const size_t n_hist = (size_t)pen.off[n_rows];
    GTR_REQUIRE(n_hist == 0 || pen.hist, "%s: %zu window ids, null list", who, n_hist);
    if (int rc = grow_upload(g_pen_dev, pens.data(), pens.size() * sizeof(PenParam))) return rc;
    if (int rc = grow_upload(g_off_dev, pen.off, ((size_t)n_rows + 1) * sizeof(int32_t))) return rc;
    const int32_t none = 0;                                                     // (no ids at all: one word nobody reads)
    if (int rc = grow_upload(g_hist_dev, n_hist ? pen.hist : &none, std::max(n_hist, (size_t)1) * sizeof(int32_t))) return rc;
    GTR_CHECK(hipStreamSynchronize(stream()));    // `pens` and `none` live on this stack frame
    return 0;
}

// the operators differ in what they take: ROWS_PLAIN no bias and no cuts, ROWS_BIASED a bias it requires, ROWS_CUT cuts and a bias it
// accepts (null: none), ROWS_PEN those and every row's window and penalty (`pen`; with pen->y_out the rows are written out and nothing
// is drawn: no request is looked at).  `who` names the operator in every message.
// ROWS_FSM (include/gten_hip_fsm.h, §3.15): ROWS_PEN without a bias, every row in a state of the caller's pool (`fsm`).
// ROWS_MIRO (include/gten_hip_mirostat.h, §3.23): ROWS_FSM without cuts, with a bias it accepts and a pool it accepts (null: no row is
// in a state), every row under its own Mirostat request (`miro`).
enum RowsLevel { ROWS_PLAIN, ROWS_BIASED, ROWS_CUT, ROWS_PEN, ROWS_FSM, ROWS_MIRO };
struct FsmRows {
    const uint16_t* next; const uint8_t* flags;      // the pool, on the device
    int n_states;
    const int32_t* state_host;                       // [n_rows]; -1: not bound
    int32_t* next_out;                               // device [n_rows] or null
};
static GrowBuf g_state_dev;                          // the rows' states of one ROWS_FSM call
static int fsm_rows_upload(const char* who, const FsmRows& f, int n_rows)
{
    GTR_REQUIRE(f.next && f.flags && f.state_host, "%s: null argument", who);
    GTR_REQUIRE(f.n_states >= 1 && f.n_states <= GTEN_HIP_FSM_MAX_STATES, "%s: a pool of %d states (1 .. %d)", who, f.n_states, GTEN_HIP_FSM_MAX_STATES);
    for (int r = 0; r < n_rows; r++)
        GTR_REQUIRE(f.state_host[r] >= -1 && f.state_host[r] < f.n_states, "%s: state %d of row %d outside [-1, %d)", who, f.state_host[r], r, f.n_states);
    return grow_upload(g_state_dev, f.state_host, (size_t)n_rows * sizeof(int32_t));
}
struct MiroRows {
    const int32_t* mu_host;                          // [n_rows] Q16
    const float *tau_host, *eta_host;                // [n_rows]; tau 0: the row draws by the routine below
    gten_hip_miro_info* info_out;                    // device [n_rows] or null
};
static GrowBuf g_miro_dev;                           // the rows' Mirostat requests of one ROWS_MIRO call
// a Mirostat request checked and converted to Q16 (the setters and the operator share the refusals)
static int miro_check(float tau, float eta, long long mu, const char* who, int* tau_q, int* eta_q)
{
    const int bad = miro_q16(tau, eta, tau_q, eta_q);
    GTR_REQUIRE(bad != MIRO_BAD_TAU, "%s: mirostat tau %g outside (0, 32]", who, (double)tau);
    GTR_REQUIRE(bad != MIRO_BAD_ETA, "%s: mirostat eta %g outside (0, 1]", who, (double)eta);
    GTR_REQUIRE(mu >= -(long long)MIRO_MU_MAX && mu <= (long long)MIRO_MU_MAX, "%s: mirostat mu %lld outside [-%d, %d] (Q16)", who, mu, MIRO_MU_MAX, MIRO_MU_MAX);
    return 0;
}
static int miro_rows_upload(const char* who, const MiroRows& m, const FsmRows& f, const float* bias, int n_rows)
{
    GTR_REQUIRE(m.mu_host && m.tau_host && m.eta_host, "%s: null argument", who);
    const bool pool = f.next || f.flags || f.state_host || f.n_states != 0;
    if (pool) {
        if (int rc = fsm_rows_upload(who, f, n_rows)) return rc;
    } else {
        const std::vector<int32_t> none((size_t)n_rows, -1);
        if (int rc = grow_upload(g_state_dev, none.data(), none.size() * sizeof(int32_t))) return rc;
        GTR_CHECK(hipStreamSynchronize(stream()));    // `none` lives on this stack frame
    }
    std::vector<MiroRowParam> rows((size_t)n_rows);
    for (int r = 0; r < n_rows; r++) {
        GTR_REQUIRE(!(bias && pool && f.state_host[r] >= 0), "%s: row %d has a bias and a state: a table and an automaton do not compose", who, r);
        MiroRowParam& q = rows[(size_t)r];
        q = MiroRowParam{m.mu_host[r], 0, 0, 0u};
        if (m.tau_host[r] == 0.f) continue;
        if (int rc = miro_check(m.tau_host[r], m.eta_host[r], m.mu_host[r], who, &q.tau_q, &q.eta_q)) return rc;
        q.on = 1u;
    }
    if (int rc = grow_upload(g_miro_dev, rows.data(), rows.size() * sizeof(MiroRowParam))) return rc;
    GTR_CHECK(hipStreamSynchronize(stream()));        // `rows` lives on this stack frame
    return 0;
}
static int sample_rows_common(const char* who, RowsLevel level, const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias,
                              long long bias_stride, const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                              const int32_t* position_host, const float* top_p_host, const float* min_p_host, int32_t* out, gten_hip_cut_info* info_out,
                              const PenRows* pen = nullptr, const FsmRows* fsm = nullptr, const MiroRows* miro = nullptr)
{
    GTR_NEED_INIT();
    const bool shape_ok = n_rows >= 0 && n_vocab >= 1 && n_vocab <= 65535 && row_stride >= 0;
    if (level == ROWS_PLAIN)
        GTR_REQUIRE(shape_ok, "%s: %d rows of %d logits (n_vocab in [1, 65535]), stride %lld", who, n_rows, n_vocab, row_stride);
    else
        GTR_REQUIRE(shape_ok && bias_stride >= 0, "%s: %d rows of %d logits (n_vocab in [1, 65535]), strides %lld, %lld", who, n_rows, n_vocab, row_stride,
                    bias_stride);
    const dim3 grid(n_rows), block(SMP_THREADS);
    if ((level == ROWS_PEN || level == ROWS_FSM) && pen->y_out) {
        GTR_REQUIRE(pen->y_stride >= n_vocab || n_rows <= 1, "%s: output stride %lld < n_vocab %d", who, pen->y_stride, n_vocab);
        if (n_rows == 0) return 0;
        GTR_REQUIRE(logits, "%s: null argument", who);
        if (int rc = pen_rows_upload(who, *pen, n_rows)) return rc;
        size_t lds = 0;
        if (level == ROWS_FSM) {
            if (int rc = fsm_rows_upload(who, *fsm, n_rows)) return rc;
            if (int rc = pen_fit((const void*)k_mask_rows_fsm, n_vocab, who, &lds)) return rc;
            GTR_LAUNCH(KT_DEC_SAMPLE, k_mask_rows_fsm, grid, block, lds, logits, n_vocab, row_stride, (const PenParam*)g_pen_dev.dev,
                       (const int32_t*)g_hist_dev.dev, (const int32_t*)g_off_dev.dev, fsm->next, fsm->flags, fsm->n_states, (const int32_t*)g_state_dev.dev,
                       pen->y_out, pen->y_stride);
            GTR_CHECK(hipStreamSynchronize(stream()));
            return 0;
        }
        if (int rc = pen_fit((const void*)k_penalize_rows, n_vocab, who, &lds)) return rc;
        GTR_LAUNCH(KT_DEC_SAMPLE, k_penalize_rows, grid, block, lds, logits, n_vocab, row_stride, bias, bias_stride, (const PenParam*)g_pen_dev.dev,
                   (const int32_t*)g_hist_dev.dev, (const int32_t*)g_off_dev.dev, pen->y_out, pen->y_stride);
        GTR_CHECK(hipStreamSynchronize(stream()));
        return 0;
    }
    if (n_rows == 0) return 0;
    const bool cutting = level == ROWS_CUT || level == ROWS_PEN || level == ROWS_FSM;
    GTR_REQUIRE(logits && out && top_k_host && temp_host && stream_host && position_host && (level != ROWS_BIASED || bias) &&
                (!cutting || (top_p_host && min_p_host)), "%s: null argument", who);
    std::vector<SampleRowParam> rows((size_t)n_rows);
    std::vector<CutParam> cuts(cutting ? (size_t)n_rows : 0);
    for (int r = 0; r < n_rows; r++) {
        if (int rc = sample_check(top_k_host[r], temp_host[r], who)) return rc;
        if (cutting)
            if (int rc = cut_check(top_p_host[r], min_p_host[r], who)) return rc;
        GTR_REQUIRE(position_host[r] >= 0, "%s: position %d of row %d", who, position_host[r], r);
        rows[(size_t)r] = SampleRowParam{top_k_host[r], temp_host[r], stream_host[r], (unsigned)position_host[r]};
        if (cutting) cuts[(size_t)r] = cut_param(top_p_host[r], min_p_host[r]);
    }
    if (level == ROWS_PEN || level == ROWS_FSM || level == ROWS_MIRO)
        if (int rc = pen_rows_upload(who, *pen, n_rows)) return rc;
    if (level == ROWS_FSM)
        if (int rc = fsm_rows_upload(who, *fsm, n_rows)) return rc;
    if (level == ROWS_MIRO)
        if (int rc = miro_rows_upload(who, *miro, *fsm, bias, n_rows)) return rc;
    if (int rc = grow_upload(g_rows_dev, rows.data(), rows.size() * sizeof(SampleRowParam))) return rc;
    const SampleRowParam* par = (const SampleRowParam*)g_rows_dev.dev;
    const unsigned seed_lo = (unsigned)(seed & 0xffffffffu), seed_hi = (unsigned)(seed >> 32);
    if (level == ROWS_MIRO) {
        size_t lds = 0;
        if (int rc = pen_fit((const void*)k_sample_rows_miro, n_vocab, who, &lds)) return rc;
        GTR_LAUNCH(KT_DEC_SAMPLE, k_sample_rows_miro, grid, block, lds, logits, n_vocab, row_stride, bias, bias_stride, par, (const PenParam*)g_pen_dev.dev,
                   (const int32_t*)g_hist_dev.dev, (const int32_t*)g_off_dev.dev, fsm->next, fsm->flags, fsm->next ? fsm->n_states : 0,
                   (const int32_t*)g_state_dev.dev, (const MiroRowParam*)g_miro_dev.dev, seed_lo, seed_hi, out, fsm->next_out, (MiroInfo*)miro->info_out);
    } else if (level == ROWS_FSM) {
        size_t lds = 0;
        if (int rc = pen_fit((const void*)k_sample_rows_fsm, n_vocab, who, &lds)) return rc;
        if (int rc = grow_upload(g_cut_dev, cuts.data(), cuts.size() * sizeof(CutParam))) return rc;
        GTR_LAUNCH(KT_DEC_SAMPLE, k_sample_rows_fsm, grid, block, lds, logits, n_vocab, row_stride, par, (const CutParam*)g_cut_dev.dev,
                   (const PenParam*)g_pen_dev.dev, (const int32_t*)g_hist_dev.dev, (const int32_t*)g_off_dev.dev, fsm->next, fsm->flags, fsm->n_states,
                   (const int32_t*)g_state_dev.dev, seed_lo, seed_hi, out, fsm->next_out, (CutInfo*)info_out);
    } else if (level == ROWS_PEN) {
        size_t lds = 0;
        if (int rc = pen_fit((const void*)k_sample_rows_pen, n_vocab, who, &lds)) return rc;
        if (int rc = grow_upload(g_cut_dev, cuts.data(), cuts.size() * sizeof(CutParam))) return rc;
        GTR_LAUNCH(KT_DEC_SAMPLE, k_sample_rows_pen, grid, block, lds, logits, n_vocab, row_stride, bias, bias_stride, par, (const CutParam*)g_cut_dev.dev,
                   (const PenParam*)g_pen_dev.dev, (const int32_t*)g_hist_dev.dev, (const int32_t*)g_off_dev.dev, seed_lo, seed_hi, out,
                   (CutInfo*)info_out);
    } else if (level == ROWS_CUT) {
        if (int rc = grow_upload(g_cut_dev, cuts.data(), cuts.size() * sizeof(CutParam))) return rc;
        GTR_LAUNCH(KT_DEC_SAMPLE, k_sample_rows_cut, grid, block, 0, logits, n_vocab, row_stride, bias, bias_stride, par, (const CutParam*)g_cut_dev.dev,
                   seed_lo, seed_hi, out, (CutInfo*)info_out);
    } else if (level == ROWS_BIASED) {
        GTR_LAUNCH(KT_DEC_SAMPLE, k_sample_rows_b, grid, block, 0, logits, n_vocab, row_stride, bias, bias_stride, par, seed_lo, seed_hi, out);
    } else {
        GTR_LAUNCH(KT_DEC_SAMPLE, k_sample_rows, grid, block, 0, logits, n_vocab, row_stride, par, seed_lo, seed_hi, out);
    }
    GTR_CHECK(hipStreamSynchronize(stream()));    // `rows` and `cuts` live on this stack frame
    return 0;
}

int gten_hip_sample_rows(const float* logits, int n_rows, int n_vocab, long long row_stride, const int32_t* top_k_host, const float* temp_host,
                         uint64_t seed, const uint32_t* stream_host, const int32_t* position_host, int32_t* out)
{
    return sample_rows_common("sample_rows", ROWS_PLAIN, logits, n_rows, n_vocab, row_stride, nullptr, 0, top_k_host, temp_host, seed, stream_host,
                              position_host, nullptr, nullptr, out, nullptr);
}

int gten_hip_sample_rows_biased(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                                const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                                const int32_t* position_host, int32_t* out)
{
    return sample_rows_common("sample_rows_biased", ROWS_BIASED, logits, n_rows, n_vocab, row_stride, bias, bias_stride, top_k_host, temp_host, seed,
                              stream_host, position_host, nullptr, nullptr, out, nullptr);
}

int gten_hip_sample_rows_cut(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                             const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                             const int32_t* position_host, const float* top_p_host, const float* min_p_host, int32_t* out,
                             gten_hip_cut_info* info_out)
{
    return sample_rows_common("sample_rows_cut", ROWS_CUT, logits, n_rows, n_vocab, row_stride, bias, bias_stride, top_k_host, temp_host, seed, stream_host,
                              position_host, top_p_host, min_p_host, out, info_out);
}

int gten_hip_penalize_rows(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                           const int32_t* hist_host, const int32_t* hist_offset_host, const float* r_host, const float* freq_host,
                           const float* pres_host, float* y_out, long long y_stride)
{
    GTR_REQUIRE(y_out && y_stride >= 0, "penalize_rows: null output or stride %lld", y_stride);
    const PenRows pen{hist_host, hist_offset_host, r_host, freq_host, pres_host, y_out, y_stride};
    return sample_rows_common("penalize_rows", ROWS_PEN, logits, n_rows, n_vocab, row_stride, bias, bias_stride, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, &pen);
}

int gten_hip_sample_rows_pen(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                             const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                             const int32_t* position_host, const float* top_p_host, const float* min_p_host, const int32_t* hist_host,
                             const int32_t* hist_offset_host, const float* r_host, const float* freq_host, const float* pres_host,
                             int32_t* out, gten_hip_cut_info* info_out)
{
    const PenRows pen{hist_host, hist_offset_host, r_host, freq_host, pres_host, nullptr, 0};
    return sample_rows_common("sample_rows_pen", ROWS_PEN, logits, n_rows, n_vocab, row_stride, bias, bias_stride, top_k_host, temp_host, seed, stream_host,
                              position_host, top_p_host, min_p_host, out, info_out, &pen);
}

int gten_hip_row_top_logprobs(const float* logits, int n_rows, int n_vocab, long long row_stride, const int32_t* ids, int n_top, float* logprob_out,
                              int32_t* top_id_out, float* top_logprob_out)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(n_vocab >= 1 && row_stride >= n_vocab, "row_top_logprobs: rows of %d logits (>= 1), stride %lld (>= n_vocab)", n_vocab, row_stride);
    GTR_REQUIRE(n_rows >= 1 && n_rows <= 65535, "row_top_logprobs: %d rows outside [1, 65535]", n_rows);
    GTR_REQUIRE(n_top >= 0 && n_top <= GTEN_HIP_LOGPROBS_TOP, "row_top_logprobs: n_top %d outside [0, %d]", n_top, GTEN_HIP_LOGPROBS_TOP);
    GTR_REQUIRE(logits && ids && logprob_out && (n_top == 0 || (top_id_out && top_logprob_out)), "row_top_logprobs: null argument");
    GTR_LAUNCH(KT_DEC_SAMPLE, k_row_top_logprobs, dim3(n_rows), dim3(SMP_THREADS), 0, logits, n_vocab, row_stride, ids, n_top, logprob_out, top_id_out,
               top_logprob_out);
    return 0;
}

// ---- token automata (include/gten_hip_fsm.h)
int gten_hip_fsm_check(const uint16_t* next_host, const uint8_t* flags_host, long long n_states, long long n_vocab, long long* where)
{
    if (where) *where = -1;
    if (!next_host || !flags_host || n_states < 1 || n_states > GTEN_HIP_FSM_MAX_STATES || n_vocab < 1) return GTEN_HIP_FSM_BAD_STATES;
    if ((unsigned long long)n_states * (unsigned long long)n_vocab * 2ull > GTEN_HIP_FSM_MAX_BYTES) return GTEN_HIP_FSM_TOO_LARGE;
    for (long long s = 0; s < n_states; s++) {
        const uint16_t* row = next_host + (size_t)s * (size_t)n_vocab;
        bool any = false;
        for (long long i = 0; i < n_vocab; i++) {
            if (row[i] == GTEN_HIP_FSM_DEAD) continue;
            if (row[i] >= n_states) { if (where) *where = s; return GTEN_HIP_FSM_BAD_ENTRY; }
            any = true;
        }
        if (!any && !(flags_host[s] & GTEN_HIP_FSM_FINAL)) { if (where) *where = s; return GTEN_HIP_FSM_STUCK; }
    }
    return GTEN_HIP_FSM_OK;
}

int gten_hip_decoder_set_fsm(gten_hip_decoder* dc, const uint16_t* next_host, const uint8_t* flags_host, int n_states)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_set_fsm: null decoder");
    GTR_REQUIRE(!dc->persist_on, "decoder_set_fsm: the persistent step (gten_hip_set_decode_persistent) has no sampler");
    SamplerState& s = dc->smp;
    GTR_REQUIRE(s.n_fsm == 0, "decoder_set_fsm: %d sequences are bound to the present pool (gten_hip_decoder_set_seq_fsm(.., -1, 0) first)", s.n_fsm);
    const bool drop = !next_host && !flags_host && n_states == 0;
    if (!drop) {
        long long where = -1;
        const int bad = gten_hip_fsm_check(next_host, flags_host, n_states, dc->d.n_vocab, &where);
        GTR_REQUIRE(bad != GTEN_HIP_FSM_BAD_STATES, "decoder_set_fsm: %d states (1 .. %d), or a null table", n_states, GTEN_HIP_FSM_MAX_STATES);
        GTR_REQUIRE(bad != GTEN_HIP_FSM_TOO_LARGE, "decoder_set_fsm: %d states of %d ids are more than %llu bytes", n_states, dc->d.n_vocab,
                    (unsigned long long)GTEN_HIP_FSM_MAX_BYTES);
        GTR_REQUIRE(bad != GTEN_HIP_FSM_BAD_ENTRY, "decoder_set_fsm: state %lld has an entry that is neither a state nor DEAD", where);
        GTR_REQUIRE(bad != GTEN_HIP_FSM_STUCK, "decoder_set_fsm: state %lld is not final and allows no id", where);
    }
    GTR_CHECK(hipStreamSynchronize(stream()));             // (no step in flight reads the pool that goes)
    uint16_t* next = nullptr;
    uint8_t* flags = nullptr;
    if (!drop) {
        // the new pool is complete on the device before the old one goes: a refusal or a failed allocation leaves the previous pool
        const size_t bytes = (size_t)n_states * (size_t)dc->d.n_vocab * sizeof(uint16_t);
        GTR_CHECK(hipMalloc((void**)&next, bytes));
        if (hipMalloc((void**)&flags, (size_t)n_states) != hipSuccess) { (void)hipFree(next); GTR_REQUIRE(false, "decoder_set_fsm: out of device memory"); }
        GTR_CHECK(hipMemcpyAsync(next, next_host, bytes, hipMemcpyHostToDevice, stream()));
        GTR_CHECK(hipMemcpyAsync(flags, flags_host, (size_t)n_states, hipMemcpyHostToDevice, stream()));
        GTR_CHECK(hipStreamSynchronize(stream()));
    }
    // (the pool's pointers and size are arguments of the captured step-end launch: graphs that hold the old ones go)
    if (s.fsm_on) GTR_CHECK(drop_graphs(dc));
    if (s.fsm_next) GTR_CHECK(hipFree(s.fsm_next));
    if (s.fsm_flags) GTR_CHECK(hipFree(s.fsm_flags));
    s.fsm_next = next; s.fsm_flags = flags; s.fsm_states = drop ? 0 : n_states;
    if (drop) s.fsm_flags_host.clear();
    else s.fsm_flags_host.assign(flags_host, flags_host + n_states);
    return 0;
}

static int fsm_make(gten_hip_decoder* dc)           // every sequence: unbound; the state rows zeroed
{
    SamplerState& s = dc->smp;
    // (this rung counts a penalised sequence's window too: its dynamic LDS limit is raised here, before any capture, whether a
    //  penalty came first or comes later -- pen_make fixes the size the launch passes)
    size_t lds = 0;
    if (int rc = pen_fit((const void*)k_dec_sample_fsm, dc->d.n_vocab, "decoder_set_seq_fsm", &lds)) return rc;
    s.fsm_host.assign((size_t)dc->n_seq, FsmParam{-1, 0, 0u, {0u, 0u, 0u, 0u, 0u}});
    const size_t rows = (size_t)dc->n_seq * (size_t)(dc->d.max_ctx + 2) * sizeof(int32_t);
    if (!s.fsm) GTR_CHECK(hipMalloc((void**)&s.fsm, (size_t)dc->n_seq * sizeof(FsmParam)));
    if (!s.fsm_state) GTR_CHECK(hipMalloc((void**)&s.fsm_state, rows));
    GTR_CHECK(hipMemcpyAsync(s.fsm, s.fsm_host.data(), s.fsm_host.size() * sizeof(FsmParam), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipMemsetAsync(s.fsm_state, 0, rows, stream()));
    return 0;
}

int gten_hip_decoder_set_seq_fsm(gten_hip_decoder* dc, int seq, int state, int pos)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && seq >= 0 && seq < dc->n_seq, "decoder_set_seq_fsm: sequence %d outside [0, %d)", seq, dc ? dc->n_seq : 0);
    SamplerState& s = dc->smp;
    if (state < 0) {
        GTR_REQUIRE(state == -1, "decoder_set_seq_fsm: state %d (-1 unbinds)", state);
        if (!s.fsm_on) return 0;                         // nobody has ever been bound: nothing to clear
        pos = 0;
    } else {
        GTR_REQUIRE(!dc->persist_on, "decoder_set_seq_fsm: the persistent step (gten_hip_set_decode_persistent) has no sampler");
        GTR_REQUIRE(s.fsm_states > 0, "decoder_set_seq_fsm: the decoder has no pool (gten_hip_decoder_set_fsm)");
        GTR_REQUIRE(state < s.fsm_states, "decoder_set_seq_fsm: state %d outside the pool's [0, %d)", state, s.fsm_states);
        GTR_REQUIRE(pos >= 1 && pos <= dc->d.max_ctx, "decoder_set_seq_fsm: position %d outside [1, %d]", pos, dc->d.max_ctx);
        GTR_REQUIRE(s.samp_host[(size_t)seq].table1 == 0,
                    "decoder_set_seq_fsm: sequence %d is bound to bias table %d (gten_hip_decoder_set_seq_bias): a table and an automaton do not compose", seq,
                    s.samp_host[(size_t)seq].table1 - 1);
        if (!s.fsm_on)
            if (int rc = first_use(dc, s.fsm_on, fsm_make)) return rc;
    }
    FsmParam& h = s.fsm_host[(size_t)seq];
    s.n_fsm += (state >= 0 ? 1 : 0) - (h.on ? 1 : 0);
    h = FsmParam{state, pos, state >= 0 ? 1u : 0u, {0u, 0u, 0u, 0u, 0u}};
    const int32_t st = state;
    if (state >= 0)
        GTR_CHECK(hipMemcpyAsync(s.fsm_state + (size_t)seq * (size_t)(dc->d.max_ctx + 2) + pos, &st, sizeof(st), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipMemcpyAsync(s.fsm + seq, &h, sizeof(FsmParam), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));
    return 0;
}

int gten_hip_decoder_fsm_info(gten_hip_decoder* dc, int* n_states, int32_t* state_host, int32_t* pos_host, int* on, int row_seq, int row_from,
                              int row_count, int32_t* row_host, const uint16_t** next_dev, const uint8_t** flags_dev)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_fsm_info: null decoder");
    const SamplerState& s = dc->smp;
    if (n_states) *n_states = s.fsm_states;
    for (int q = 0; q < dc->n_seq; q++) {
        const bool b = s.fsm_on && s.fsm_host[(size_t)q].on != 0u;
        if (state_host) state_host[q] = b ? s.fsm_host[(size_t)q].state : -1;
        if (pos_host) pos_host[q] = b ? s.fsm_host[(size_t)q].pos : 0;
    }
    if (on) *on = s.fsm_on ? 1 : 0;
    if (next_dev) *next_dev = s.fsm_next;
    if (flags_dev) *flags_dev = s.fsm_flags;
    if (row_host) {
        GTR_REQUIRE(row_seq >= 0 && row_seq < dc->n_seq && row_from >= 0 && row_count >= 0 && row_from + row_count <= dc->d.max_ctx + 2,
                    "decoder_fsm_info: entries [%d, %d + %d) of sequence %d's state row (%d entries, %d sequences)", row_from, row_from, row_count, row_seq,
                    dc->d.max_ctx + 2, dc->n_seq);
        if (!s.fsm_state) std::fill(row_host, row_host + row_count, 0);
        else if (row_count > 0) {
            GTR_CHECK(hipStreamSynchronize(stream()));
            GTR_CHECK(hipMemcpy(row_host, s.fsm_state + (size_t)row_seq * (size_t)(dc->d.max_ctx + 2) + row_from, (size_t)row_count * 4, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

int gten_hip_decoder_slot_states(gten_hip_decoder* dc, int seq, int n_from, int count, int32_t* states_host)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && states_host && seq >= 0 && seq < dc->n_seq, "decoder_slot_states: bad arguments");
    GTR_REQUIRE(n_from >= 0 && count >= 0 && n_from + count <= dc->d.max_ctx + 2, "decoder_slot_states: entries [%d, %d) outside [0, %d)", n_from, n_from + count,
                dc->d.max_ctx + 2);
    GTR_REQUIRE(dc->smp.fsm_state, "decoder_slot_states: no sequence of this decoder has been bound to an automaton (gten_hip_decoder_set_seq_fsm)");
    GTR_CHECK(hipStreamSynchronize(stream()));
    if (count > 0)
        GTR_CHECK(hipMemcpy(states_host, dc->smp.fsm_state + (size_t)seq * (size_t)(dc->d.max_ctx + 2) + n_from, (size_t)count * 4, hipMemcpyDeviceToHost));
    return 0;
}

// the penalties of an automaton operator's rows: the caller's, or "none" for every row when it passes no window offsets
struct FsmPenDefaults {
    std::vector<int32_t> off;
    std::vector<float> one, zero;
    PenRows rows(int n_rows, const int32_t* hist, const int32_t* off_host, const float* r, const float* freq, const float* pres, float* y_out, long long y_stride)
    {
        if (off_host) return PenRows{hist, off_host, r, freq, pres, y_out, y_stride};
        off.assign((size_t)std::max(n_rows, 0) + 1, 0);
        one.assign((size_t)std::max(n_rows, 1), 1.f);
        zero.assign((size_t)std::max(n_rows, 1), 0.f);
        return PenRows{nullptr, off.data(), one.data(), zero.data(), zero.data(), y_out, y_stride};
    }
};

int gten_hip_mask_rows_fsm(const float* logits, int n_rows, int n_vocab, long long row_stride, const uint16_t* next, const uint8_t* flags, int n_states,
                           const int32_t* state_host, const int32_t* hist_host, const int32_t* hist_offset_host, const float* r_host,
                           const float* freq_host, const float* pres_host, float* y_out, long long y_stride)
{
    GTR_REQUIRE(y_out && y_stride >= 0, "mask_rows_fsm: null output or stride %lld", y_stride);
    FsmPenDefaults d;
    const PenRows pen = d.rows(n_rows, hist_host, hist_offset_host, r_host, freq_host, pres_host, y_out, y_stride);
    const FsmRows fsm{next, flags, n_states, state_host, nullptr};
    return sample_rows_common("mask_rows_fsm", ROWS_FSM, logits, n_rows, n_vocab, row_stride, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, &pen, &fsm);
}

int gten_hip_sample_rows_fsm(const float* logits, int n_rows, int n_vocab, long long row_stride, const uint16_t* next, const uint8_t* flags, int n_states,
                             const int32_t* state_host, const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                             const int32_t* position_host, const float* top_p_host, const float* min_p_host, const int32_t* hist_host,
                             const int32_t* hist_offset_host, const float* r_host, const float* freq_host, const float* pres_host, int32_t* out,
                             int32_t* next_state_out, gten_hip_cut_info* info_out)
{
    FsmPenDefaults d;
    const PenRows pen = d.rows(n_rows, hist_host, hist_offset_host, r_host, freq_host, pres_host, nullptr, 0);
    const FsmRows fsm{next, flags, n_states, state_host, next_state_out};
    return sample_rows_common("sample_rows_fsm", ROWS_FSM, logits, n_rows, n_vocab, row_stride, nullptr, 0, top_k_host, temp_host, seed, stream_host,
                              position_host, top_p_host, min_p_host, out, info_out, &pen, &fsm);
}

// ---- Mirostat v2 (include/gten_hip_mirostat.h)
// the shared arithmetic, device-free: no GTR_NEED_INIT
int32_t gten_hip_miro_lg16_host(uint64_t x) { return (int32_t)miro_lg16((unsigned long long)x); }
int32_t gten_hip_miro_update_host(int32_t mu, int32_t s, int32_t tau_q, int32_t eta_q) { return (int32_t)miro_update(mu, s, tau_q, eta_q); }
int gten_hip_miro_q16_host(float tau, float eta, int32_t* tau_q, int32_t* eta_q)
{
    int t = 0, e = 0;
    const int bad = miro_q16(tau, eta, &t, &e);
    if (bad != MIRO_OK) return bad;
    if (tau_q) *tau_q = t;
    if (eta_q) *eta_q = e;
    return GTEN_HIP_MIRO_OK;
}
static_assert(MIRO_OK == GTEN_HIP_MIRO_OK && MIRO_BAD_TAU == GTEN_HIP_MIRO_BAD_TAU && MIRO_BAD_ETA == GTEN_HIP_MIRO_BAD_ETA,
              "gten_miro_math.h and include/gten_hip_mirostat.h disagree");

static int miro_make(gten_hip_decoder* dc)          // every sequence: unbound; the mu rows zeroed
{
    SamplerState& s = dc->smp;
    // (this rung counts a penalised sequence's window too: its dynamic LDS limit is raised here, before any capture, as fsm_make does)
    size_t lds = 0;
    if (int rc = pen_fit((const void*)k_dec_sample_miro, dc->d.n_vocab, "decoder_set_seq_mirostat", &lds)) return rc;
    s.miro_host.assign((size_t)dc->n_seq, MiroParam{0, 0, 0, 0u});
    const size_t rows = (size_t)dc->n_seq * (size_t)(dc->d.max_ctx + 2) * sizeof(int32_t);
    if (!s.miro) GTR_CHECK(hipMalloc((void**)&s.miro, (size_t)dc->n_seq * sizeof(MiroParam)));
    if (!s.miro_mu) GTR_CHECK(hipMalloc((void**)&s.miro_mu, rows));
    GTR_CHECK(hipMemcpyAsync(s.miro, s.miro_host.data(), s.miro_host.size() * sizeof(MiroParam), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipMemsetAsync(s.miro_mu, 0, rows, stream()));
    return 0;
}

int gten_hip_decoder_set_seq_mirostat(gten_hip_decoder* dc, int seq, float tau, float eta, int32_t mu_q16, int pos)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && seq >= 0 && seq < dc->n_seq, "decoder_set_seq_mirostat: sequence %d outside [0, %d)", seq, dc ? dc->n_seq : 0);
    SamplerState& s = dc->smp;
    MiroParam h{0, 0, 0, 0u};
    int32_t mu = 0;
    if (tau == 0.f) {
        if (!s.miro_on) return 0;                        // nobody has ever been bound: nothing to clear
    } else {
        if (int rc = miro_check(tau, eta, mu_q16 == GTEN_HIP_MIRO_MU_DEFAULT ? 0 : (long long)mu_q16, "decoder_set_seq_mirostat", &h.tau_q, &h.eta_q)) return rc;
        mu = mu_q16 == GTEN_HIP_MIRO_MU_DEFAULT ? 2 * h.tau_q : mu_q16;
        GTR_REQUIRE(!dc->persist_on, "decoder_set_seq_mirostat: the persistent step (gten_hip_set_decode_persistent) has no sampler");
        GTR_REQUIRE(pos >= 1 && pos <= dc->d.max_ctx, "decoder_set_seq_mirostat: position %d outside [1, %d]", pos, dc->d.max_ctx);
        GTR_REQUIRE(!s.cut_on || s.cut_host[(size_t)seq].on == 0u,
                    "decoder_set_seq_mirostat: sequence %d draws under a cut (gten_hip_decoder_set_cut): a cut and mirostat do not compose", seq);
        if (!s.miro_on)
            if (int rc = first_use(dc, s.miro_on, miro_make)) return rc;
        h.pos = pos; h.on = 1u;
    }
    s.miro_host[(size_t)seq] = h;
    if (h.on)
        GTR_CHECK(hipMemcpyAsync(s.miro_mu + (size_t)seq * (size_t)(dc->d.max_ctx + 2) + pos, &mu, sizeof(mu), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipMemcpyAsync(s.miro + seq, &s.miro_host[(size_t)seq], sizeof(MiroParam), hipMemcpyHostToDevice, stream()));
    GTR_CHECK(hipStreamSynchronize(stream()));           // `mu` lives on this stack frame
    return 0;
}

// entries [from, from + count) of sequence seq's mu row to the host (zeros while nobody has ever been bound)
static int miro_row_read(gten_hip_decoder* dc, const char* who, int seq, int from, int count, int32_t* out_host)
{
    GTR_REQUIRE(seq >= 0 && seq < dc->n_seq && from >= 0 && count >= 0 && from + count <= dc->d.max_ctx + 2,
                "%s: entries [%d, %d + %d) of sequence %d's mu row (%d entries, %d sequences)", who, from, from, count, seq, dc->d.max_ctx + 2, dc->n_seq);
    if (count == 0) return 0;
    GTR_REQUIRE(out_host, "%s: null output", who);
    if (!dc->smp.miro_mu) { std::fill(out_host, out_host + count, 0); return 0; }
    GTR_CHECK(hipStreamSynchronize(stream()));
    GTR_CHECK(hipMemcpy(out_host, dc->smp.miro_mu + (size_t)seq * (size_t)(dc->d.max_ctx + 2) + from, (size_t)count * 4, hipMemcpyDeviceToHost));
    return 0;
}

int gten_hip_decoder_mirostat_info(gten_hip_decoder* dc, int32_t* tau_q_host, int32_t* eta_q_host, int32_t* pos_host, int* on, int row_seq,
                                   int row_from, int row_count, int32_t* row_host)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc, "decoder_mirostat_info: null decoder");
    const SamplerState& s = dc->smp;
    for (int q = 0; q < dc->n_seq; q++) {
        const MiroParam m = s.miro_on ? s.miro_host[(size_t)q] : MiroParam{0, 0, 0, 0u};
        if (tau_q_host) tau_q_host[q] = m.on ? m.tau_q : 0;
        if (eta_q_host) eta_q_host[q] = m.on ? m.eta_q : 0;
        if (pos_host) pos_host[q] = m.on ? m.pos : 0;
    }
    if (on) *on = s.miro_on ? 1 : 0;
    if (row_host) return miro_row_read(dc, "decoder_mirostat_info", row_seq, row_from, row_count, row_host);
    return 0;
}

int gten_hip_decoder_slot_mus(gten_hip_decoder* dc, int seq, int n_from, int count, int32_t* out_host)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(dc && out_host, "decoder_slot_mus: null argument");
    return miro_row_read(dc, "decoder_slot_mus", seq, n_from, count, out_host);
}

int gten_hip_sample_rows_miro(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                              const uint16_t* next, const uint8_t* flags, int n_states, const int32_t* state_host, const int32_t* top_k_host,
                              const float* temp_host, uint64_t seed, const uint32_t* stream_host, const int32_t* position_host,
                              const int32_t* hist_host, const int32_t* hist_offset_host, const float* r_host, const float* freq_host,
                              const float* pres_host, const int32_t* mu_host, const float* tau_host, const float* eta_host, int32_t* out,
                              int32_t* next_state_out, gten_hip_miro_info* info_out)
{
    FsmPenDefaults d;
    const PenRows pen = d.rows(n_rows, hist_host, hist_offset_host, r_host, freq_host, pres_host, nullptr, 0);
    const FsmRows fsm{next, flags, n_states, state_host, next_state_out};
    const MiroRows miro{mu_host, tau_host, eta_host, info_out};
    return sample_rows_common("sample_rows_miro", ROWS_MIRO, logits, n_rows, n_vocab, row_stride, bias, bias_stride, top_k_host, temp_host, seed, stream_host,
                              position_host, nullptr, nullptr, out, nullptr, &pen, &fsm, &miro);
}
