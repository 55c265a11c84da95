// pce_whisper_selftest.inc -- the pce_selftest_* entry points (include/pce.h) and their helpers, included by pce_whisper_impl.inc: its kernels on host arrays.
namespace {
// pce_selftest_gemm_tiled: the kernel a selector stands for (GK_AUTO: the product's rule), or -1 where that kernel does not compute the shape
template <int EPI> static int selftest_gemm_kind(const pce_ctx *c, int kernel, const GemmShape &s)
{
    const int kind = kernel == GK_AUTO ? gemm_choose<EPI>(c, s) : kernel;
    return gemm_fits<EPI>(kind, s) ? kind : -1;
}

// pce_selftest_layernorm's k_add_layernorm forms: the stream is updated in place when it keeps its type (as the encoder runs it), else written to
// a second buffer
template <class OUT, class RIN, class ROUT>
static int selftest_add_layernorm(pce_ctx *c, int64_t rows, int d, const void *x, const uint16_t *delta, const uint16_t *delta2, const float *w, const float *b,
                                  float eps, int write_resid, void *out, void *resid_out, uint16_t *out_copy)
{
    constexpr bool IN_PLACE = std::is_same<RIN, ROUT>::value;
    const size_t n = (size_t)rows * d;
    DevBuf din, dres, ddl, ddl2, dw, db, dout, dcopy;
    PCE_UPLOAD(c, din, static_cast<const RIN *>(x), n); PCE_UPLOAD(c, ddl, delta, n); PCE_UPLOAD(c, dw, w, (size_t)d); PCE_UPLOAD(c, db, b, (size_t)d);
    if (delta2) PCE_UPLOAD(c, ddl2, delta2, n);
    PCE_ZERO(OUT, c, dout, n);
    if (!IN_PLACE) PCE_ZERO(ROUT, c, dres, n);
    if (out_copy) PCE_ZERO(uint16_t, c, dcopy, n);
    ROUT *rout = IN_PLACE ? din.as<ROUT>() : dres.as<ROUT>();
    launch_add_layernorm<OUT, RIN, ROUT>(c, din.as<RIN>(), rout, ddl.as<op_t>(), delta2 ? ddl2.as<op_t>() : nullptr, write_resid, dw.as<float>(), db.as<float>(),
                                         rows, d, dout.as<OUT>(), eps, out_copy ? dcopy.as<op_t>() : nullptr);
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, static_cast<OUT *>(out), dout.p, n);
    if (resid_out) PCE_FETCH(c, static_cast<ROUT *>(resid_out), rout, n);
    if (out_copy) PCE_FETCH(c, out_copy, dcopy.p, n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

// pce_selftest_encoder_walk's probe: behind a launch of encoder_walk, a device-to-device copy, on the walk's stream, of the buffer(s) that launch wrote into
// layer l's part of the capture buffers (their layout: include/pce.h).  The first copy that fails is kept.
struct WalkCapture {
    pce_ctx *c; const EncoderRun *r; bool pre_ln;
    op_t *ln16, *qk, *vt, *attn, *hidden; float *x32;
    size_t Md, MI, nvt;                                          // elements of a [M][d] buffer, of r.hidden, of r.vt
    hipError_t *failed;
    void keep(void *dst, const void *src, size_t bytes) const
    {
        if (*failed == hipSuccess) *failed = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream);
    }
    void operator()(int l, EncoderStage s) const
    {
        const size_t y = (size_t)l, b16 = sizeof(op_t), b32 = sizeof(float);
        op_t *ln_at = ln16 + y * 3 * Md;
        float *x_at = x32 + y * 4 * Md;
        switch (s) {
        case ES_LN_A: keep(ln_at, r->ln, b16 * Md); break;
        case ES_QKV: keep(qk + y * 2 * Md, r->qk, b16 * 2 * Md); keep(vt + y * nvt, r->vt, b16 * nvt); break;
        case ES_ATTN: keep(attn + y * Md, r->attn, b16 * Md); break;
        case ES_X1: keep(x_at, r->resid, b32 * Md); break;
        case ES_LN_B: keep(ln_at + Md, r->ln, b16 * Md); if (!pre_ln) keep(x_at + Md, r->resid, b32 * Md); break;
        case ES_HIDDEN: keep(hidden + y * MI, r->hidden, b16 * MI); break;
        case ES_X2: keep(x_at + 2 * Md, r->resid, b32 * Md); break;
        case ES_LN_C: keep(ln_at + 2 * Md, r->ln, b16 * Md); keep(x_at + 3 * Md, r->resid, b32 * Md); break;
        }
    }
};
// encoder_walk<W2vGemm> under that probe: defined at the end of pce_w2v.inc, where wav2vec2's GEMM rule is
static bool selftest_walk_w2v(pce_ctx *c, const EncoderRun &r, const std::vector<EncoderLayerW> &layers, bool pre_ln, const WalkCapture &probe);
} // namespace

// V rows of clip c at rows k_row0[c] .. + k_len[c] of [.][heads * 64] -> the V^T image the attention kernels read: [clip][head * 64 + d][sp] (the
// rest of the key axis keeps its zeros)
static __global__ void k_selftest_vt(const op_t *__restrict__ v, const int *__restrict__ k_row0, const int *__restrict__ k_len, int hd, int sp,
                                     op_t *__restrict__ vt)
{
    const int clip = blockIdx.y;
    const int64_t n = (int64_t)k_len[clip] * hd;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % hd), t = (int)(i / hd);
        vt[((int64_t)clip * hd + col) * sp + t] = v[(int64_t)k_row0[clip] * hd + i];
    }
}

namespace PCE_BUILD_NS {

// Self-test hooks of the attention kernel through launch_attention (see pce.h)
int pce_selftest_attention_ragged(pce_ctx *c, const uint16_t *q, const uint16_t *k, const uint16_t *v, int32_t clips, int32_t heads, const int32_t *q_len,
                                  const int32_t *k_len, int32_t causal, int32_t mode, uint16_t *out, int64_t out_rows, int32_t *fell_back)
{
    if (!c || !q || !k || !v || !out || !q_len || !k_len || clips <= 0 || clips > 65535 || heads <= 0 || heads > 65535 || mode < 0 || mode > 1)
        return PCE_E_INVALID;
    std::vector<int> tab((size_t)4 * clips);
    int64_t q_rows = 0, k_rows = 0;
    int q_max = 0, k_max = 0;
    for (int i = 0; i < clips; i++) {
        if (q_len[i] < 1 || k_len[i] < 1 || q_len[i] > (1 << 20) || k_len[i] > (1 << 20)) return pce_fail(c, PCE_E_INVALID, "selftest attention: clip %d has %d queries, %d keys", i, q_len[i], k_len[i]);
        tab[(size_t)i] = (int)q_rows; tab[(size_t)clips + i] = q_len[i]; tab[(size_t)2 * clips + i] = (int)k_rows; tab[(size_t)3 * clips + i] = k_len[i];
        q_rows += q_len[i]; k_rows += k_len[i];
        q_max = q_len[i] > q_max ? q_len[i] : q_max; k_max = k_len[i] > k_max ? k_len[i] : k_max;
    }
    const int hd = heads * 64, sp = div_up(k_max, 64) * 64;
    if (out_rows < q_rows || (out_rows + k_rows) * hd >= ((int64_t)1 << 30)) return pce_fail(c, PCE_E_INVALID, "selftest attention: %lld output rows for %lld queries", (long long)out_rows, (long long)q_rows);
    PCE_HIP(c, hipSetDevice(c->device));
    const size_t nq = (size_t)q_rows * hd, nk = (size_t)k_rows * hd, nvt = (size_t)clips * hd * sp, no = (size_t)out_rows * hd;
    DevBuf dq, dk, dv, dvt, dout, dtab, dcnt;
    PCE_UPLOAD(c, dq, q, nq, 32); PCE_UPLOAD(c, dk, k, nk, 32); PCE_UPLOAD(c, dv, v, nk, 32); PCE_UPLOAD(c, dout, out, no, 32); PCE_UPLOAD(c, dtab, tab);
    PCE_ZERO(uint16_t, c, dvt, nvt + 64);
    PCE_ZERO(int, c, dcnt, 1);
    AttnArgs a{};
    a.q = dq.as<op_t>(); a.q_ld = hd; a.k = dk.as<op_t>(); a.k_ld = hd; a.vt = dvt.as<op_t>(); a.vt_clip = (int64_t)hd * sp; a.vt_sp = sp;
    a.q_row0 = dtab.as<int>(); a.q_len = a.q_row0 + clips; a.k_row0 = a.q_row0 + 2 * clips; a.k_len = a.q_row0 + 3 * clips;
    a.out = dout.as<op_t>(); a.out_ld = hd; a.causal = causal; a.fell_back = dcnt.as<int>();
    hipLaunchKernelGGL(k_selftest_vt, dim3((unsigned)div_up((int64_t)k_max * hd, 256), (unsigned)clips), dim3(256), 0, c->stream, dv.as<op_t>(), a.k_row0,
                       a.k_len, hd, sp, dvt.as<op_t>());
    // the grid of the longest clip, as the teacher-forced decoder launches it: one query block takes the NT instantiation
    launch_attention(c, dim3((unsigned)div_up(q_max, AT_QB), (unsigned)heads, (unsigned)clips), a, 0.0, mode);
    PCE_HIP(c, hipGetLastError());
    int cnt = 0;
    PCE_FETCH(c, out, dout.p, no);
    PCE_FETCH(c, &cnt, dcnt.p, 1);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    if (fell_back) *fell_back = cnt;
    return PCE_OK;
}
int pce_selftest_attention(pce_ctx *c, const uint16_t *q, const uint16_t *k, const uint16_t *v, int32_t clips, int32_t heads, int32_t q_len,
                           int32_t k_len, int32_t causal, int32_t mode, uint16_t *out, int32_t *fell_back)
{
    if (!c || !out || clips <= 0 || heads <= 0 || q_len <= 0 || k_len <= 0) return PCE_E_INVALID;
    const std::vector<int32_t> ql((size_t)clips, q_len), kl((size_t)clips, k_len);
    std::fill(out, out + (size_t)clips * q_len * heads * 64, (uint16_t)0);
    return PCE_BUILD_NS::pce_selftest_attention_ragged(c, q, k, v, clips, heads, ql.data(), kl.data(), causal, mode, out, (int64_t)clips * q_len, fell_back);
}

// Self-test hook of the single-query attention kernels of an incremental decoding step, through the launches the step makes (see pce.h)
int pce_selftest_attn1(pce_ctx *c, int32_t form, int32_t n, int32_t heads, const uint16_t *q, int64_t q_elems, uint16_t *k, int64_t k_elems, uint16_t *v,
                       int64_t v_elems, const int32_t *k_row0, const int32_t *len, const int32_t *skip, int32_t span, uint16_t *out, int64_t out_elems)
{
    if (!c || form < 0 || form > 2 || !q || !k || !v || !len || !out || n < 1 || n > 65535 || heads < 1 || span < 1) return PCE_E_INVALID;
    if (heads > 32) return pce_fail(c, PCE_E_INVALID, "selftest attn1: %d heads (the kernels hold 32)", heads);
    const int64_t d = (int64_t)heads * 64;
    const int T_cap = span, vt_sp = form == 0 ? span : 512;
    if (form == 0 && (!k_row0 || vt_sp % 8 != 0)) return pce_fail(c, PCE_E_INVALID, "selftest attn1: form 0 needs k_row0 and vt_sp %% 8 == 0 (%d)", vt_sp);
    if (form != 0 && T_cap > 512) return pce_fail(c, PCE_E_INVALID, "selftest attn1: T_cap %d > 512", T_cap);
    const int64_t q_need = (int64_t)n * d * (form == 0 ? 1 : 3), v_need = (int64_t)n * d * (form == 2 ? T_cap : vt_sp), o_need = (int64_t)n * d;
    int64_t k_need = form == 0 ? 0 : (int64_t)n * T_cap * d;
    std::vector<int> tab((size_t)4 * n, 0);                        // k_row0 | k_len | pos | skip
    for (int i = 0; i < n; i++) {
        if (form == 0) {
            if (len[i] < 1 || len[i] > 1536 || k_row0[i] < 0 || (len[i] + 7) / 8 * 8 > vt_sp)
                return pce_fail(c, PCE_E_INVALID, "selftest attn1: clip %d has %d keys from row %d (V^T pitch %d)", i, len[i], k_row0[i], vt_sp);
            const int64_t end = ((int64_t)k_row0[i] + len[i]) * d;
            k_need = end > k_need ? end : k_need;
            tab[(size_t)i] = k_row0[i]; tab[(size_t)n + i] = len[i];
        } else {
            if (len[i] < 0 || len[i] >= T_cap) return pce_fail(c, PCE_E_INVALID, "selftest attn1: clip %d at position %d of %d", i, len[i], T_cap);
            tab[(size_t)i] = i * T_cap; tab[(size_t)n + i] = len[i] + 1; tab[(size_t)2 * n + i] = len[i];
        }
        tab[(size_t)3 * n + i] = skip ? skip[i] : 0;
    }
    if (q_elems < q_need || k_elems < k_need || v_elems < v_need || out_elems < o_need || k_elems >= ((int64_t)1 << 31) || v_elems >= ((int64_t)1 << 31))
        return pce_fail(c, PCE_E_INVALID, "selftest attn1: form %d needs q %lld, k %lld, v %lld, out %lld elements", form, (long long)q_need, (long long)k_need,
                        (long long)v_need, (long long)o_need);
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(lds_optins(c, ws_of(c)));
    DevBuf dq, dk, dv, dout, dtab;
    PCE_UPLOAD(c, dq, q, (size_t)q_elems, 32); PCE_UPLOAD(c, dk, k, (size_t)k_elems, 32); PCE_UPLOAD(c, dv, v, (size_t)v_elems, 32);
    PCE_UPLOAD(c, dout, out, (size_t)out_elems, 32); PCE_UPLOAD(c, dtab, tab);
    const int *T = dtab.as<int>(), *SKIP = skip ? T + 3 * n : nullptr;
    if (form == 2) {
        SelfAttn1Args sa{};
        sa.qkv = dq.as<op_t>(); sa.qkv_ld = 3 * d; sa.ck = dk.as<op_t>(); sa.cv = dv.as<op_t>(); sa.c_clip = (int64_t)T_cap * d; sa.d = (int)d;
        sa.pos = T + 2 * n; sa.skip = SKIP; sa.out = dout.as<op_t>(); sa.out_ld = d;
        launch_self_attn1(c, n, heads, sa);
    } else {
        Attn1Args a{};
        a.q = dq.as<op_t>(); a.q_ld = form == 0 ? d : 3 * d; a.k = dk.as<op_t>(); a.k_ld = d; a.vt = dv.as<op_t>(); a.vt_clip = d * vt_sp; a.vt_sp = vt_sp;
        a.k_row0 = T; a.k_len = T + n; a.skip = SKIP; a.out = dout.as<op_t>(); a.out_ld = d;
        if (form == 1) { a.app_k = dq.as<op_t>() + d; a.app_v = dq.as<op_t>() + 2 * d; a.app_ld = 3 * d; a.app_pos = T + 2 * n; }
        launch_cross_attn1(c, n, heads, a);
    }
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, out, dout.p, (size_t)out_elems);
    if (form != 0) { PCE_FETCH(c, k, dk.p, (size_t)k_elems); PCE_FETCH(c, v, dv.p, (size_t)v_elems); }
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

// Self-test hook of the forced alignment's matrix kernels (k_align_scores, k_align_colnorm, k_align_cost<7> / <0>) through the launches
// pce_whisper_align_run makes (launch_align_scores once or twice, as one or two layers would, then launch_align_cost), with the shapes padded by the
// run's own code.  See include/pce.h.
int pce_selftest_align_matrix(pce_ctx *c, int32_t n, int32_t heads, const uint16_t *q, int64_t q_elems, const uint16_t *k, int64_t k_elems, int32_t k_rows,
                              const int32_t *t_len, const int32_t *f_len, const int32_t *heads_sel, int32_t n_sel, int32_t split, int32_t sot_len,
                              int32_t medfilt_width, float qk_scale, float *w_soft, int64_t w_soft_elems, float *w_norm, int64_t w_norm_elems, double *cost,
                              int64_t cost_elems)
{
    if (!c || !q || !k || !t_len || !f_len || !heads_sel || !w_soft || !w_norm || !cost || n < 1 || n > 65535 || heads < 1 || n_sel < 1 || n_sel > 65535 || sot_len < 0)
        return PCE_E_INVALID;
    if (heads > 32) return pce_fail(c, PCE_E_INVALID, "selftest align: %d heads (a decoder holds 32)", heads);
    if (!align_width_ok(medfilt_width)) return pce_fail(c, PCE_E_INVALID, "median filter width must be odd, <= 15");
    if (split < 0 || split > n_sel) return pce_fail(c, PCE_E_INVALID, "selftest align: split %d of %d selected heads", split, n_sel);
    if (k_rows < 1 || k_rows > W_CTX) return pce_fail(c, PCE_E_INVALID, "selftest align: %d key rows per clip (1..%d)", k_rows, W_CTX);
    for (int s = 0; s < n_sel; s++)
        if (heads_sel[s] < 0 || heads_sel[s] >= heads) return pce_fail(c, PCE_E_INVALID, "selftest align: selected head %d of %d", heads_sel[s], heads);
    AlignDims dims;
    int T_max = 0;
    for (int i = 0; i < n; i++) {
        if (f_len[i] > k_rows) return pce_fail(c, PCE_E_INVALID, "selftest align: clip %d has %d frames, %d key rows", i, f_len[i], k_rows);
        PCE_TRY(align_clip_dims(c, i, t_len[i], f_len[i], sot_len, 448, dims));                               // (448: the longest n_text_ctx a decoder loads with)
        T_max = std::max(T_max, t_len[i]);
    }
    const int d = heads * 64, T_pad = token_rows_pad(T_max), F_pad = dims.F_pad(), N_max = dims.N_max;
    const int64_t q_need = (int64_t)n * T_pad * d, k_need = (int64_t)n * k_rows * d, w_need = (int64_t)n * n_sel * T_pad * F_pad, c_need = (int64_t)n * N_max * F_pad;
    if (q_elems < q_need || k_elems < k_need || w_soft_elems < w_need || w_norm_elems < w_need || cost_elems < c_need || w_need >= ((int64_t)1 << 28))
        return pce_fail(c, PCE_E_INVALID, "selftest align: needs q %lld, k %lld, w_soft / w_norm %lld, cost %lld elements", (long long)q_need, (long long)k_need,
                        (long long)w_need, (long long)c_need);
    PCE_HIP(c, hipSetDevice(c->device));
    std::vector<int> tab((size_t)2 * n + n_sel);                  // t_len | f_len | heads
    for (int i = 0; i < n; i++) { tab[(size_t)i] = t_len[i]; tab[(size_t)n + i] = f_len[i]; }
    for (int s = 0; s < n_sel; s++) tab[(size_t)2 * n + s] = heads_sel[s];
    DevBuf dq, dk, dw, dc, dtab;
    const size_t k_clip = (size_t)W_CTX * d;                      // the key pitch k_align_scores assumes: 1500 rows per clip
    PCE_UPLOAD(c, dq, q, (size_t)q_need, 32);
    PCE_ZERO(uint16_t, c, dk, k_clip * (size_t)n, 32);
    PCE_HIP(c, hipMemcpy2DAsync(dk.p, 2 * k_clip, k, 2 * (size_t)k_rows * d, 2 * (size_t)k_rows * d, (size_t)n, hipMemcpyHostToDevice, c->stream));
    PCE_UPLOAD(c, dw, w_soft, (size_t)w_need); PCE_UPLOAD(c, dc, cost, (size_t)c_need); PCE_UPLOAD(c, dtab, tab);
    const int *TL = dtab.as<int>(), *FL = TL + n, *HS = TL + 2 * n;
    const AlignMatrix am{dw.as<float>(), TL, FL, n, n_sel, T_pad, F_pad};
    const int first = split == 0 ? n_sel : split;                // heads of the first launch (the rest: a second layer's)
    launch_align_scores(c, am, dq.as<op_t>(), dk.as<op_t>(), d, HS, 0, first, qk_scale);
    if (first < n_sel) launch_align_scores(c, am, dq.as<op_t>(), dk.as<op_t>(), d, HS, first, n_sel - first, qk_scale);
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, w_soft, dw.p, (size_t)w_need);
    launch_align_cost(c, am, sot_len, medfilt_width, N_max, dc.as<double>());
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, w_norm, dw.p, (size_t)w_need);
    PCE_FETCH(c, cost, dc.p, (size_t)c_need);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

// Self-test hook of the kernels that turn a decoding step's logits into tokens (k_decode_rules, k_step_advance) on host arrays, through launch_decode_rules /
// launch_step_advance, which decode_step_device and pce_whisper_decode_loop make their launches with: no model is loaded.  form 0: ONE launch over the prompts
// padded to T_pad, as decode_step_device; form 1: `steps` times the rules at the table's pitch t_cap, then k_step_advance, as the loop.  The log-probability is
// -log(sum exp(x - x[choice])) over what the filters leave: a sampled choice more than about 88 below the maximum overflows the sum and reads -inf.
// See include/pce.h.
int pce_selftest_decode_rules(pce_ctx *c, int32_t form, int32_t n, int32_t n_vocab, int32_t steps, const float *logits, int64_t logits_elems, const int32_t *tokens,
                              const int32_t *token_offsets, int32_t pad_token, int32_t t_cap, const int32_t *sample_begin, int32_t sample_begin_all,
                              const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, int64_t mask_elems, float temperature, uint32_t seed_lo,
                              uint32_t seed_hi, int32_t probe_token, const int32_t *sample_keys, int32_t max_new, int32_t *out_tok, float *out_lp,
                              float *probe_prob, int64_t out_elems, int32_t *table, int64_t table_elems, int32_t *loop_state, int64_t state_elems)
{
    if (!c) return PCE_E_INVALID;
    if (form < 0 || form > 1 || !logits || !tokens || !token_offsets || !rules || !vocab_mask || !out_tok || !out_lp || n < 1 || n > 65535 || steps < 1)
        return pce_fail(c, PCE_E_INVALID, "selftest decode rules: form 0 or 1, 1 <= n <= 65535, steps >= 1, and logits, tokens, token_offsets, rules, vocab_mask, out_tok, out_lp given");
    if (form == 0 && (!probe_prob || steps != 1)) return pce_fail(c, PCE_E_INVALID, "selftest decode rules: form 0 is one step with probe_prob");
    if (form == 1 && (!table || !loop_state || max_new < 1 || steps > max_new))
        return pce_fail(c, PCE_E_INVALID, "selftest decode rules: form 1 needs table, loop_state and 1 <= steps <= max_new");
    const int V = n_vocab;
    if (V < 1 || V > DR_K * DR_T) return pce_fail(c, PCE_E_INVALID, "selftest decode rules: n_vocab %d (1..%d)", V, DR_K * DR_T);
    if (rules->eot < 0 || rules->eot >= V || rules->timestamp_begin <= rules->eot || rules->timestamp_begin > V)
        return pce_fail(c, PCE_E_INVALID, "decoding rules: need 0 <= eot < timestamp_begin <= n_vocab, sample_begin >= 1");
    if (!(temperature >= 0.f) || probe_token >= V) return pce_fail(c, PCE_E_INVALID, "decoding options: temperature >= 0, probe_token < n_vocab");
    if (t_cap < 1 || t_cap > 448) return pce_fail(c, PCE_E_INVALID, "selftest decode rules: t_cap %d (1..448)", t_cap);
    const int64_t ld = div_up(V, 128) * 128;
    int T_max = 0;
    std::vector<int> h_len((size_t)n), h_sb((size_t)n);
    for (int i = 0; i < n; i++) {
        const int T = token_offsets[i + 1] - token_offsets[i], sb = sample_begin ? sample_begin[i] : sample_begin_all;
        if (sb < 1 || T < sb || T > t_cap) return pce_fail(c, PCE_E_INVALID, "clip %d: %d tokens (need %d..%d)", i, T, sb, t_cap);
        for (int t = 0; t < T; t++) {
            const int v = tokens[token_offsets[i] + t];
            if (v < 0 || v >= V) return pce_fail(c, PCE_E_INVALID, "token %d out of the vocabulary", v);
        }
        h_len[(size_t)i] = T; h_sb[(size_t)i] = sb; T_max = std::max(T_max, T);
    }
    const int pitch = form == 0 ? token_rows_pad(T_max) : t_cap;
    const int64_t logits_need = (int64_t)steps * n * ld, out_need = form == 0 ? n : (int64_t)n * max_new, table_need = form == 0 ? 0 : (int64_t)n * t_cap,
                  state_need = form == 0 ? 0 : (int64_t)10 * n + max_new + 1;
    if (logits_elems < logits_need || mask_elems < V || out_elems < out_need || table_elems < table_need || state_elems < state_need || logits_elems >= ((int64_t)1 << 30) ||
        out_elems >= ((int64_t)1 << 28) || table_elems >= ((int64_t)1 << 28) || state_elems >= ((int64_t)1 << 28))
        return pce_fail(c, PCE_E_INVALID, "selftest decode rules: form %d needs logits %lld, vocab_mask %d, outputs %lld, table %lld, loop_state %lld elements", form,
                        (long long)logits_need, V, (long long)out_need, (long long)table_need, (long long)state_need);
    PCE_HIP(c, hipSetDevice(c->device));
    // the token rows: the prompts at the launch's pitch; what lies past a sequence's length is pad_token (form 0) or what the caller's table holds (form 1)
    std::vector<int> h_tok;
    if (form == 0) h_tok.assign((size_t)n * pitch, pad_token); else h_tok.assign(table, table + table_elems);
    for (int i = 0; i < n; i++) memcpy(&h_tok[(size_t)i * pitch], &tokens[token_offsets[i]], sizeof(int) * (size_t)h_len[(size_t)i]);
    DevBuf dlog, dtok, dlen, dsb, dmask, dkeys, dout, dlp, dprobe, dstate, dnext;
    PCE_UPLOAD(c, dlog, logits, (size_t)logits_elems); PCE_UPLOAD(c, dtok, h_tok); PCE_UPLOAD(c, dsb, h_sb); PCE_UPLOAD(c, dmask, vocab_mask, (size_t)V, 64);
    PCE_UPLOAD(c, dout, out_tok, (size_t)out_elems); PCE_UPLOAD(c, dlp, out_lp, (size_t)out_elems);
    if (sample_keys) PCE_UPLOAD(c, dkeys, sample_keys, (size_t)n);
    const int *keys = sample_keys ? dkeys.as<int>() : nullptr;
    DecRules R{rules->eot, rules->timestamp_begin, V, (int)ld, sample_begin_all, rules->max_initial_timestamp_index, temperature, seed_lo, seed_hi,
               form == 0 && probe_token >= 0 ? probe_token : -1};
    if (form == 0) {
        PCE_UPLOAD(c, dprobe, probe_prob, (size_t)out_elems); PCE_UPLOAD(c, dlen, h_len);
        launch_decode_rules(c, n, dlog.as<float>(), dtok.as<int>(), dlen.as<int>(), pitch, dmask.as<unsigned char>(), R, dsb.as<int>(), dout.as<int>(), dlp.as<float>(),
                            dprobe.as<float>(), keys);
        PCE_HIP(c, hipGetLastError());
        PCE_FETCH(c, probe_prob, dprobe.p, (size_t)out_elems);
    } else {
        // loop_state: len [n] | ended [n] | ct [8 n] | n_ended [max_new] | step counter.  The lengths are the prompts', the counts and the counter start at zero (as the
        // loop's do); ended and ct come in with the caller's values
        std::vector<int> h_state(loop_state, loop_state + state_elems);
        memcpy(h_state.data(), h_len.data(), sizeof(int) * (size_t)n);
        std::fill(h_state.begin() + (size_t)10 * n, h_state.begin() + (size_t)state_need, 0);
        PCE_UPLOAD(c, dstate, h_state); PCE_HIP(c, dnext.reserve((sizeof(int) + sizeof(float)) * (size_t)n));
        PCE_HIP(c, hipStreamSynchronize(c->stream));              // (h_state leaves scope below)
        int *S = dstate.as<int>(), *next = dnext.as<int>();
        float *next_lp = reinterpret_cast<float *>(next + n);
        const DecodeLoopState state{dtok.as<int>(), S, S + n, dout.as<int>(), dlp.as<float>(), S + (size_t)10 * n + max_new, S + (size_t)10 * n};
        for (int s = 0; s < steps; s++) {
            launch_decode_rules(c, n, dlog.as<float>() + (size_t)s * n * (size_t)ld, state.tok_table, state.len, pitch, dmask.as<unsigned char>(), R, dsb.as<int>(), next,
                                next_lp, nullptr, keys);
            launch_step_advance(c, state, n, t_cap, (int)rules->eot, (int)max_new, next, next_lp, S + (size_t)2 * n);
        }
        PCE_HIP(c, hipGetLastError());
        PCE_FETCH(c, table, dtok.p, (size_t)table_elems);
        PCE_FETCH(c, loop_state, dstate.p, (size_t)state_elems);
    }
    PCE_FETCH(c, out_tok, dout.p, (size_t)out_elems);
    PCE_FETCH(c, out_lp, dlp.p, (size_t)out_elems);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

// Self-test hook of the encoder-output cross-attention of an incremental decoding step (pce_xattn.inc): k_xq_fused -> k_xattn_absorbed -> k_uv_absorb of ONE
// layer on host arrays, with the number of workgroups per clip forced (0: what the batch size selects).  See include/pce.h.
// pce_selftest_xattn_stages adds the skip list and copies out what the launch leaves between its kernels: Q' (hi | lo), the nodes' U and (m, l).  Every DevBuf
// frees itself on the early returns of PCE_HIP (pce_internal.h).
int pce_selftest_xattn_stages(pce_ctx *c, const float *resid, const float *ln_w, const float *ln_b, const uint16_t *wq, const float *bq, const uint16_t *wk,
                              const uint16_t *wv, const float *bv, const uint16_t *E, int64_t e_elems, const int32_t *k_len, const int32_t *skip, int32_t n,
                              int32_t k_cap, int32_t d, int32_t heads, int32_t workgroups_per_clip, uint16_t *out, int64_t out_elems, uint16_t *qp_hi,
                              uint16_t *qp_lo, int64_t qp_elems, float *u_part, int64_t u_elems, float *ml_part, int64_t ml_elems, int32_t *nodes_out)
{
    if (!c || !resid || !ln_w || !ln_b || !wq || !bq || !wk || !wv || !bv || !E || !k_len || !out || n <= 0 || k_cap <= 0) return PCE_E_INVALID;
    if (!xa_has_form(d, heads))
        return pce_fail(c, PCE_E_INVALID, "selftest xattn: d = %d with %d heads is not a width the encoder-output form is built for", d, heads);
    if (!(workgroups_per_clip == 0 || workgroups_per_clip == 1 || workgroups_per_clip == 2 || workgroups_per_clip == 4)) return PCE_E_INVALID;
    for (int i = 0; i < n; i++) if (k_len[i] <= 0 || k_len[i] > k_cap) return pce_fail(c, PCE_E_INVALID, "selftest xattn: clip %d has %d frames of %d", i, k_len[i], k_cap);
    const size_t dd = (size_t)d * d, ne = (size_t)n * k_cap * d;
    const size_t R = (size_t)xa_rows(heads);
    const int nsplit = xa_split(n, workgroups_per_clip);
    // the nodes xattn_launch_d will write: the pair form (two) where the width has it and a workgroup owns both leaves of a pair, else the four leaves
    const int nodes = (d <= 768 && nsplit <= XA_LEAVES / 2) ? XA_LEAVES / 2 : XA_LEAVES;
    const size_t nqp = (size_t)n * R * d, nup = (size_t)n * nodes * R * d, nml = (size_t)n * nodes * R * 2;
    if ((qp_hi != nullptr) != (qp_lo != nullptr) || (u_part != nullptr) != (ml_part != nullptr)) return PCE_E_INVALID;
    if (e_elems < (int64_t)ne || out_elems < (int64_t)n * d || (qp_hi && qp_elems < (int64_t)nqp) || (u_part && (u_elems < (int64_t)nup || ml_elems < (int64_t)nml)))
        return pce_fail(c, PCE_E_INVALID, "selftest xattn: needs E %lld, out %lld, qp_hi / qp_lo %lld, u_part %lld, ml_part %lld elements",
                        (long long)ne, (long long)n * d, (long long)nqp, (long long)nup, (long long)nml);
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(lds_optins(c, ws_of(c)));
    DevBuf dres, dlw, dlb, dwq, dbq, dwk, dwkT, dwv, dbv, dE, dkl, dqp, dup, dml, dout;
    const size_t nd = (size_t)n * d, w = (size_t)d;
    PCE_UPLOAD(c, dres, resid, nd); PCE_UPLOAD(c, dlw, ln_w, w); PCE_UPLOAD(c, dlb, ln_b, w); PCE_UPLOAD(c, dwq, wq, dd); PCE_UPLOAD(c, dbq, bq, w);
    PCE_UPLOAD(c, dwk, wk, dd); PCE_UPLOAD(c, dwv, wv, dd); PCE_UPLOAD(c, dbv, bv, w); PCE_UPLOAD(c, dE, E, ne, 2048); PCE_UPLOAD(c, dout, out, nd, 32);
    PCE_UPLOAD(c, dkl, k_len, (size_t)n, (size_t)n);             // k_len | skip
    PCE_HIP(c, dwkT.reserve(2 * dd)); PCE_HIP(c, dqp.reserve(2 * 2 * nqp + 256)); PCE_HIP(c, dup.reserve(sizeof(float) * (size_t)n * XA_MAX_SPLIT * R * d + 256));
    PCE_HIP(c, dml.reserve(sizeof(float) * (size_t)n * XA_MAX_SPLIT * R * 2 + 256));
    op_t *QH = dqp.as<op_t>(), *QL = QH + nqp;
    if (qp_hi) { PCE_PUT(c, QH, qp_hi, nqp); PCE_PUT(c, QL, qp_lo, nqp); }
    else PCE_HIP(c, hipMemsetAsync(dqp.p, 0, dqp.cap, c->stream));
    if (u_part) { PCE_PUT(c, dup.p, u_part, nup); PCE_PUT(c, dml.p, ml_part, nml); }
    if (skip) PCE_PUT(c, dkl.as<int>() + n, skip, (size_t)n);
    hipLaunchKernelGGL(k_transpose_sq, dim3((unsigned)(d / 32), (unsigned)(d / 32)), dim3(256), 0, c->stream, dwk.as<op_t>(), dwkT.as<op_t>(), d);
    XaArgs a{};
    a.E = dE.as<op_t>(); a.e_clip = (int64_t)k_cap * d; a.e_ld = d; a.k_len = dkl.as<int>(); a.skip = skip ? dkl.as<int>() + n : nullptr;
    a.u_part = dup.as<float>(); a.ml_part = dml.as<float>(); a.heads = heads; a.nsplit = nsplit; a.rows = (int)R;
    XaLayer y{};
    y.resid = dres.as<float>(); y.ln_w = dlw.as<float>(); y.ln_b = dlb.as<float>(); y.wq = dwq.as<op_t>(); y.bq = dbq.as<float>(); y.wkT = dwkT.as<op_t>();
    y.wv = dwv.as<op_t>(); y.bv = dbv.as<float>(); y.qp_hi = QH; y.qp_lo = QL; y.out = dout.as<op_t>(); y.out_ld = d;
    xattn_launch(c, d, n, a, y);
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, out, dout.p, nd);
    if (qp_hi) { PCE_FETCH(c, qp_hi, QH, nqp); PCE_FETCH(c, qp_lo, QL, nqp); }
    if (u_part) { PCE_FETCH(c, u_part, dup.p, nup); PCE_FETCH(c, ml_part, dml.p, nml); }
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    if (nodes_out) *nodes_out = nodes;
    return PCE_OK;
}
int pce_selftest_xattn(pce_ctx *c, const float *resid, const float *ln_w, const float *ln_b, const uint16_t *wq, const float *bq, const uint16_t *wk,
                       const uint16_t *wv, const float *bv, const uint16_t *E, const int32_t *k_len, int32_t n, int32_t k_cap, int32_t d, int32_t heads,
                       int32_t workgroups_per_clip, uint16_t *out)
{
    if (!c || !out || n <= 0 || k_cap <= 0 || d <= 0) return PCE_E_INVALID;
    std::fill(out, out + (size_t)n * d, (uint16_t)0);
    return PCE_BUILD_NS::pce_selftest_xattn_stages(c, resid, ln_w, ln_b, wq, bq, wk, wv, bv, E, (int64_t)n * k_cap * d, k_len, nullptr, n, k_cap, d, heads,
                                                   workgroups_per_clip, out, (int64_t)n * d, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, nullptr);
}

// Self-test hook of the persistent 256 x 256 GEMM: C = epilogue(A B^T + bias) on host arrays (op_t bit patterns in, op_t bit patterns out).
// epilogue 0: bias, 1: bias + GELU, 2: bias, written transposed per clip (rows_per_clip rows, key axis padded to vt_sp): out[(clip N + n) vt_sp + t]
int pce_selftest_gemm(pce_ctx *c, const uint16_t *A, const uint16_t *B, const float *bias, int32_t M, int32_t N, int32_t K, int32_t epilogue,
                      int32_t rows_per_clip, int32_t vt_sp, uint16_t *out)
{
    if (!c || !A || !B || !out || M <= 0 || N <= 0 || K <= 0) return PCE_E_INVALID;
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(lds_optins(c, ws_of(c)));
    if (epilogue >= 16 && epilogue <= 19) {
        // the tiled / few-row kernels behind launch_gemm (which of them runs follows from the shape and PCE_GEMM_SKINNY; pce_selftest_gemm_tiled
        // chooses one and takes every epilogue): 16 = bias,
        // 17 = bias + GELU (16-bit outputs), 19 = accumulate into a zeroed fp32 matrix (out receives M * N floats)
        const bool f32 = epilogue == 19;
        DevBuf tA, tB, tC, tb;
        PCE_UPLOAD(c, tA, A, (size_t)M * K, 2048);
        PCE_ZERO(uint16_t, c, tB, (size_t)(N + 128) * K, 2048); PCE_PUT(c, tB.p, B, (size_t)N * K);
        PCE_ZERO(float, c, tb, (size_t)(N + 128));
        if (bias) PCE_PUT(c, tb.p, bias, (size_t)N);
        PCE_ZERO(float, c, tC, (size_t)M * N, 1024);
        if (N % 128) return pce_fail(c, PCE_E_INVALID, "selftest gemm (tiled): N must be a multiple of 128");
        c->gemm_few_rows = true;                                   // (the few-row kernel is eligible here, as in an incremental decoding step)
        struct Off { pce_ctx *c; ~Off() { c->gemm_few_rows = false; } } off{c};
        if (epilogue == 16) launch_gemm<EPI_BF16>(c, tA.as<op_t>(), K, 0, tB.as<op_t>(), M, N, K, tb.as<float>(), tC.p, N, 0, 1);
        else if (epilogue == 17) launch_gemm<EPI_GELU_BF16>(c, tA.as<op_t>(), K, 0, tB.as<op_t>(), M, N, K, tb.as<float>(), tC.p, N, 0, 1);
        else if (epilogue == 19) launch_gemm<EPI_RESID_F32>(c, tA.as<op_t>(), K, 0, tB.as<op_t>(), M, N, K, tb.as<float>(), tC.p, N, 0, 1);
        else return pce_fail(c, PCE_E_INVALID, "selftest gemm: epilogue 18 does not exist");
        PCE_HIP(c, hipGetLastError());
        if (f32) PCE_FETCH(c, reinterpret_cast<float *>(out), tC.p, (size_t)M * N);
        else PCE_FETCH(c, out, tC.p, (size_t)M * N);
        PCE_HIP(c, hipStreamSynchronize(c->stream));
        pce_profile_collect(c);
        return PCE_OK;
    }
    const size_t n_out = epilogue == 2 ? (size_t)(M / rows_per_clip) * N * vt_sp
                         : epilogue >= 256 ? (size_t)M * epilogue + (size_t)(M / rows_per_clip) * (N - epilogue) * vt_sp : (size_t)M * N;
    DevBuf dA, dB, dC, dbias;
    PCE_UPLOAD(c, dA, A, (size_t)M * K); PCE_UPLOAD(c, dB, B, (size_t)N * K);
    if (bias) PCE_UPLOAD(c, dbias, bias, (size_t)N);
    PCE_ZERO(uint16_t, c, dC, n_out);
    bool ok = false;
    const float *bp = bias ? dbias.as<float>() : nullptr;
    if (epilogue == 0) ok = launch_gemm_flat<FEPI_BF16>(c, dA.as<op_t>(), dB.as<op_t>(), bp, dC.as<op_t>(), M, N, K, N);
    else if (epilogue == 1) ok = launch_gemm_flat<FEPI_GELU>(c, dA.as<op_t>(), dB.as<op_t>(), bp, dC.as<op_t>(), M, N, K, N);
    else if (epilogue == 2) ok = launch_gemm_flat<FEPI_VT>(c, dA.as<op_t>(), dB.as<op_t>(), bp, dC.as<op_t>(), M, N, K, 0, rows_per_clip, vt_sp);
    else if (epilogue >= 256 && epilogue % 256 == 0 && epilogue < N)      // split launch: columns [0, epilogue) row-major [M][epilogue], then the V^T image of the rest
        ok = launch_gemm_flat<FEPI_SPLIT>(c, dA.as<op_t>(), dB.as<op_t>(), bp, dC.as<op_t>(), M, N, K, epilogue, rows_per_clip, vt_sp, PCE_K_GEMM_FLAT,
                                          dC.as<op_t>() + (size_t)M * epilogue, epilogue);
    int rc = ok ? PCE_OK : pce_fail(c, PCE_E_LIMIT, "shape not handled by the 256 x 256 kernel (N %% 256, K %% 64)");
    if (ok) rc = [&]() -> int { PCE_HIP(c, hipGetLastError()); PCE_FETCH(c, out, dC.p, n_out); PCE_HIP(c, hipStreamSynchronize(c->stream)); return PCE_OK; }();
    (void)hipStreamSynchronize(c->stream);
    pce_profile_collect(c);
    return rc;
}

// Self-test hook of the persistent 256 x 256 GEMM's residual epilogue (FEPI_RESID), in place as the encoder runs it:
// resid_inout[M][N] = r16(resid_inout + r16(A B^T + bias)), 16-bit bit patterns of the context's operand type.
int pce_selftest_gemm_resid(pce_ctx *c, const uint16_t *A, const uint16_t *B, const float *bias, uint16_t *resid_inout, int32_t M, int32_t N, int32_t K)
{
    if (!c || !A || !B || !resid_inout || M <= 0 || N <= 0 || K <= 0) return PCE_E_INVALID;
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(lds_optins(c, ws_of(c)));
    DevBuf dA, dB, dC, dbias;
    PCE_UPLOAD(c, dA, A, (size_t)M * K); PCE_UPLOAD(c, dB, B, (size_t)N * K); PCE_UPLOAD(c, dC, resid_inout, (size_t)M * N);
    if (bias) PCE_UPLOAD(c, dbias, bias, (size_t)N);
    const bool ok = launch_gemm_flat<FEPI_RESID>(c, dA.as<op_t>(), dB.as<op_t>(), bias ? dbias.as<float>() : nullptr, dC.as<op_t>(), M, N, K, N, 1, 0, PCE_K_GEMM_FLAT,
                                                 nullptr, 0, dC.as<op_t>());
    int rc = ok ? PCE_OK : pce_fail(c, PCE_E_LIMIT, "shape not handled by the 256 x 256 kernel (N %% 256, K %% 64)");
    if (ok) rc = [&]() -> int { PCE_HIP(c, hipGetLastError()); PCE_FETCH(c, resid_inout, dC.p, (size_t)M * N); PCE_HIP(c, hipStreamSynchronize(c->stream)); return PCE_OK; }();
    (void)hipStreamSynchronize(c->stream);
    pce_profile_collect(c);
    return rc;
}

// Self-test hook of the tiled / few-row GEMM kernels through the product's own launch code (launch_gemm_kernel; see pce.h).  Every byte a launch
// can address is checked against the caller's buffer lengths before anything is allocated.
int pce_selftest_gemm_tiled(pce_ctx *c, int32_t kernel, int32_t epilogue, const uint16_t *A, int64_t a_len, int64_t lda, int64_t a_batch, int32_t batch,
                            const uint16_t *B, const float *bias, int32_t M, int32_t N, int32_t K, void *C, int64_t c_len, int64_t ldc, int64_t c_batch,
                            const float *pos, int32_t pos_T, int32_t v_col0, int32_t rows_per_clip, int32_t vt_sp, uint16_t *vt, int64_t vt_len,
                            int32_t *kernel_used)
{
    if (!c || !A || !B || !C || M <= 0 || N <= 0 || K <= 0 || batch <= 0 || kernel < GK_AUTO || kernel > GK_128_DEEP || epilogue < EPI_BF16 || epilogue > EPI_F32)
        return PCE_E_INVALID;
    const bool f32 = epilogue == EPI_GELU_POS_F32 || epilogue == EPI_RESID_F32 || epilogue == EPI_F32, qkv = epilogue == EPI_QKV;
    const int64_t nc = qkv ? v_col0 : N;                                 // row-major output columns
    if (lda < 1 || lda % 8 || a_batch < 0 || a_batch % 8 || ldc < nc || ldc % 8 || c_batch < 0 || c_batch % 8)
        return pce_fail(c, PCE_E_INVALID, "selftest gemm (tiled): lda, a_batch, ldc, c_batch must be multiples of 8 (16-byte rows), ldc >= the output columns");
    if ((int64_t)(batch - 1) * a_batch + (int64_t)(M - 1) * lda + K > a_len)
        return pce_fail(c, PCE_E_INVALID, "selftest gemm (tiled): A holds %lld elements, the shape reads beyond them", (long long)a_len);
    if (nc > 0 && (int64_t)(batch - 1) * c_batch + (int64_t)(M - 1) * ldc + nc > c_len)
        return pce_fail(c, PCE_E_INVALID, "selftest gemm (tiled): C holds %lld elements, the shape writes beyond them", (long long)c_len);
    if (epilogue == EPI_GELU_POS_F32 && (!pos || pos_T < 1)) return pce_fail(c, PCE_E_INVALID, "selftest gemm (tiled): GELU_POS_F32 needs pos [pos_T][N]");
    int64_t n_vt = 0;
    if (qkv) {
        // V columns [v_col0, N) leave as vt[clip][column - v_col0][t] (clip = row / rows_per_clip, t < rows_per_clip <= vt_sp): four rows per store
        const int S = rows_per_clip;
        if (!vt || batch != 1 || v_col0 < 0 || v_col0 >= N || (N - v_col0) % 64 || S < 4 || S % 4 || vt_sp < S || vt_sp % 4)
            return pce_fail(c, PCE_E_INVALID, "selftest gemm (tiled): QKV needs vt, batch 1, 0 <= v_col0 < N, rows_per_clip %% 4 == 0, rows_per_clip <= vt_sp, vt_sp %% 4 == 0");
        n_vt = (int64_t)div_up(M, S) * (N - v_col0) * vt_sp;
        if (n_vt > vt_len) return pce_fail(c, PCE_E_INVALID, "selftest gemm (tiled): vt holds %lld elements, the V image needs %lld", (long long)vt_len, (long long)n_vt);
    }
    const GemmShape s{M, N, K, lda, batch, qkv ? v_col0 : 0};
    // refuse what the chosen kernel cannot compute before any allocation
    const int kind = epilogue == EPI_BF16 ? selftest_gemm_kind<EPI_BF16>(c, kernel, s) : epilogue == EPI_GELU_BF16 ? selftest_gemm_kind<EPI_GELU_BF16>(c, kernel, s)
                     : epilogue == EPI_GELU_POS_F32 ? selftest_gemm_kind<EPI_GELU_POS_F32>(c, kernel, s) : epilogue == EPI_RESID_F32 ? selftest_gemm_kind<EPI_RESID_F32>(c, kernel, s)
                     : epilogue == EPI_QKV ? selftest_gemm_kind<EPI_QKV>(c, kernel, s) : selftest_gemm_kind<EPI_F32>(c, kernel, s);
    if (kind < 0)
        return pce_fail(c, PCE_E_LIMIT, "selftest gemm (tiled): kernel %d does not compute epilogue %d at M %d x N %d x K %d (lda %lld, batch %d, v_col0 %d)",
                        kernel, epilogue, M, N, K, (long long)lda, batch, v_col0);
    if (kernel_used) *kernel_used = kind;
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(lds_optins(c, ws_of(c)));
    DevBuf dA, dB, dbias, dC, dpos, dvt;
    PCE_UPLOAD(c, dA, A, (size_t)a_len); PCE_UPLOAD(c, dB, B, (size_t)N * K);
    // C goes in as well: read by RESID_F32, kept where nothing is written (16 bytes of slack)
    if (f32) PCE_UPLOAD(c, dC, static_cast<const float *>(C), (size_t)c_len, 4);
    else PCE_UPLOAD(c, dC, static_cast<const uint16_t *>(C), (size_t)c_len, 8);
    if (bias) PCE_UPLOAD(c, dbias, bias, (size_t)N);
    if (epilogue == EPI_GELU_POS_F32) PCE_UPLOAD(c, dpos, pos, (size_t)pos_T * N);
    if (qkv) PCE_UPLOAD(c, dvt, vt, (size_t)vt_len);
    const op_t *a = dA.as<op_t>(), *b = dB.as<op_t>();
    const float *bp = bias ? dbias.as<float>() : nullptr;
    switch (epilogue) {
    case EPI_BF16: launch_gemm_kernel<EPI_BF16>(c, kind, a, lda, a_batch, b, M, N, K, bp, dC.p, ldc, c_batch, batch, nullptr, 1, 0, 0); break;
    case EPI_GELU_BF16: launch_gemm_kernel<EPI_GELU_BF16>(c, kind, a, lda, a_batch, b, M, N, K, bp, dC.p, ldc, c_batch, batch, nullptr, 1, 0, 0); break;
    case EPI_GELU_POS_F32: launch_gemm_kernel<EPI_GELU_POS_F32>(c, kind, a, lda, a_batch, b, M, N, K, bp, dC.p, ldc, c_batch, batch, dpos.as<float>(), pos_T, 0, 0); break;
    case EPI_RESID_F32: launch_gemm_kernel<EPI_RESID_F32>(c, kind, a, lda, a_batch, b, M, N, K, bp, dC.p, ldc, c_batch, batch, nullptr, 1, 0, 0); break;
    case EPI_QKV:        // (the V^T image travels in the pos argument, its clip length in pos_T: as the product launches it)
        launch_gemm_kernel<EPI_QKV>(c, kind, a, lda, a_batch, b, M, N, K, bp, dC.p, ldc, c_batch, batch, reinterpret_cast<const float *>(dvt.as<op_t>()),
                                    rows_per_clip, v_col0, vt_sp);
        break;
    default: launch_gemm_kernel<EPI_F32>(c, kind, a, lda, a_batch, b, M, N, K, bp, dC.p, ldc, c_batch, batch, nullptr, 1, 0, 0); break;
    }
    PCE_HIP(c, hipGetLastError());
    if (f32) PCE_FETCH(c, static_cast<float *>(C), dC.p, (size_t)c_len);
    else PCE_FETCH(c, static_cast<uint16_t *>(C), dC.p, (size_t)c_len);
    if (qkv) PCE_FETCH(c, vt, dvt.p, (size_t)vt_len);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

// Self-test hook of the LayerNorm kernels (k_layernorm, k_add_layernorm) as the product launches them (launch_layernorm / launch_add_layernorm; see pce.h)
int pce_selftest_layernorm(pce_ctx *c, int32_t form, int32_t rows, int32_t d, const void *x, const uint16_t *delta, const uint16_t *delta2, const float *w,
                           const float *b, float eps, int32_t flags, void *out, void *resid_out, uint16_t *out_copy)
{
    if (!c || !x || !w || !b || !out || rows <= 0 || form < 0 || form > 7) return PCE_E_INVALID;
    if (d < 4 || d % 4 || d > LN_D_MAX) return pce_fail(c, PCE_E_LIMIT, "selftest layernorm: d = %d (need d %% 4 == 0, d <= %d)", d, LN_D_MAX);
    PCE_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)rows * d;
    if (form <= 1) {
        // k_layernorm<float | op_t>; flags bit 0: round_in16, bit 1: out2 = x (in place, as the BERT layers write their fp32 stream), returned in resid_out
        const bool in_place = flags & 2;
        if (in_place && !resid_out) return PCE_E_INVALID;
        DevBuf dx, dw, db, dout;
        PCE_UPLOAD(c, dx, static_cast<const float *>(x), n); PCE_UPLOAD(c, dw, w, (size_t)d); PCE_UPLOAD(c, db, b, (size_t)d);
        if (form) PCE_ZERO(uint16_t, c, dout, n); else PCE_ZERO(float, c, dout, n);
        float *o2 = in_place ? dx.as<float>() : nullptr;
        if (form) launch_layernorm<op_t>(c, dx.as<float>(), dw.as<float>(), db.as<float>(), rows, d, dout.as<op_t>(), eps, o2, flags & 1);
        else launch_layernorm<float>(c, dx.as<float>(), dw.as<float>(), db.as<float>(), rows, d, dout.as<float>(), eps, o2, flags & 1);
        PCE_HIP(c, hipGetLastError());
        if (form) PCE_FETCH(c, static_cast<uint16_t *>(out), dout.p, n); else PCE_FETCH(c, static_cast<float *>(out), dout.p, n);
        if (in_place) PCE_FETCH(c, static_cast<float *>(resid_out), dx.p, n);
        PCE_HIP(c, hipStreamSynchronize(c->stream));
        return PCE_OK;
    }
    // k_add_layernorm<OUT, RIN, ROUT>: form 2 + 3 o + s, o = 0: fp32 output, 1: 16-bit output; s = 0: fp32 stream, 1: fp32 in / 16-bit out, 2: 16-bit stream.
    // flags bit 2: write_resid
    if (!delta) return PCE_E_INVALID;
    const int o = (form - 2) / 3, st = (form - 2) % 3, wr = (flags >> 2) & 1;
    if (o == 0) {
        if (st == 0) return selftest_add_layernorm<float, float, float>(c, rows, d, x, delta, delta2, w, b, eps, wr, out, resid_out, out_copy);
        if (st == 1) return selftest_add_layernorm<float, float, op_t>(c, rows, d, x, delta, delta2, w, b, eps, wr, out, resid_out, out_copy);
        return selftest_add_layernorm<float, op_t, op_t>(c, rows, d, x, delta, delta2, w, b, eps, wr, out, resid_out, out_copy);
    }
    if (st == 0) return selftest_add_layernorm<op_t, float, float>(c, rows, d, x, delta, delta2, w, b, eps, wr, out, resid_out, out_copy);
    if (st == 1) return selftest_add_layernorm<op_t, float, op_t>(c, rows, d, x, delta, delta2, w, b, eps, wr, out, resid_out, out_copy);
    return selftest_add_layernorm<op_t, op_t, op_t>(c, rows, d, x, delta, delta2, w, b, eps, wr, out, resid_out, out_copy);
}

// Self-test hook of the shared encoder layer walk (encoder_walk, pce_encoder.inc) on host arrays: the weights go through pack_encoder_layer and
// upload_weights as a loader's do, the EncoderRun is filled as pce_whisper_encode_run (pre_ln, rule 0), pce_bert_run (post-LN, rule 0) and w2v_forward_chunk
// (rule 1) fill theirs, and the walk's probe copies out, behind every launch, the buffer that launch wrote.  See include/pce.h.
int pce_selftest_encoder_walk(pce_ctx *c, int32_t pre_ln, int32_t gemm_rule, int32_t key_bias, int32_t d, int32_t heads, int32_t inner, int32_t n_layers,
                              int32_t n_items, int32_t rows_per_item, int32_t vt_sp, const int32_t *len, float eps, const float *weights, int64_t n_floats,
                              const float *stream, int64_t stream_elems, const uint16_t *ln_in, uint16_t *ln16, int64_t ln16_elems, uint16_t *qk, int64_t qk_elems,
                              uint16_t *vt, int64_t vt_elems, uint16_t *attn, int64_t attn_elems, uint16_t *hidden, int64_t hidden_elems, float *x32,
                              int64_t x32_elems, int32_t *fit_out)
{
    if (!c || !len || !weights || !stream || !ln16 || !qk || !vt || !attn || !hidden || !x32 || pre_ln < 0 || pre_ln > 1 || gemm_rule < 0 || gemm_rule > 1 ||
        key_bias < 0 || key_bias > 1 || n_layers < 1 || n_layers > 2 || n_items < 1 || n_items > 65535)
        return PCE_E_INVALID;
    if (!pre_ln && !ln_in) return pce_fail(c, PCE_E_INVALID, "selftest encoder walk: a post-LN stack needs ln_in, the 16-bit image its opening LayerNorm leaves");
    // what the three loaders refuse
    if (d <= 0 || d % 128 || heads * 64 != d) return pce_fail(c, PCE_E_LIMIT, "selftest encoder walk: d %d with %d heads (need d %% 128 == 0, head size 64)", d, heads);
    if (d > LN_D_MAX) return pce_fail(c, PCE_E_LIMIT, "selftest encoder walk: d %d: the LayerNorm kernels hold at most %d", d, LN_D_MAX);
    if (inner <= 0 || inner % 128) return pce_fail(c, PCE_E_LIMIT, "selftest encoder walk: inner %d is no multiple of 128 (the GEMM's column tile)", inner);
    // an item's slot: the QKV epilogue stores four rows at a time, the attention reads V^T in 64-key tiles
    if (rows_per_item < 4 || rows_per_item % 4 || vt_sp % 64 || rows_per_item > vt_sp || vt_sp > (1 << 20))
        return pce_fail(c, PCE_E_INVALID, "selftest encoder walk: %d rows per item in %d V^T columns (need rows %% 4 == 0, columns %% 64 == 0, rows <= columns)",
                        rows_per_item, vt_sp);
    for (int i = 0; i < n_items; i++)
        if (len[i] < 1 || len[i] > rows_per_item) return pce_fail(c, PCE_E_INVALID, "selftest encoder walk: item %d has %d rows of %d", i, len[i], rows_per_item);
    const int64_t M = (int64_t)n_items * rows_per_item, L = n_layers, I = inner;
    const int64_t Md = M * d, MI = M * I, nvt = (int64_t)n_items * d * vt_sp;
    if (M * std::max<int64_t>(2 * d, I) >= ((int64_t)1 << 30) || nvt >= ((int64_t)1 << 30))
        return pce_fail(c, PCE_E_LIMIT, "selftest encoder walk: %lld rows are more than the self-test holds", (long long)M);
    const int64_t per_layer = 4LL * d * d + (key_bias ? 4LL : 3LL) * d + 2LL * d + (I * d + I) + (d * I + d) + 2LL * d;
    if (n_floats != L * per_layer)
        return pce_fail(c, PCE_E_INVALID, "selftest encoder walk: weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)(L * per_layer));
    if (stream_elems < Md || ln16_elems < L * 3 * Md || qk_elems < L * 2 * Md || vt_elems < L * nvt || attn_elems < L * Md || hidden_elems < L * MI || x32_elems < L * 4 * Md)
        return pce_fail(c, PCE_E_INVALID, "selftest encoder walk: needs stream %lld, ln16 %lld, qk %lld, vt %lld, attn %lld, hidden %lld, x32 %lld elements", (long long)Md,
                        (long long)(L * 3 * Md), (long long)(L * 2 * Md), (long long)(L * nvt), (long long)(L * Md), (long long)(L * MI), (long long)(L * 4 * Md));
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(lds_optins(c, ws_of(c)));
    // the loader's half: openai-whisper's tensor order for the Whisper encoder (the pre-LN stack on the product's rule), transformers' for BERT and wav2vec2
    const bool pre = pre_ln != 0, whisper = pre && gemm_rule == 0;
    WeightPack pk;
    std::vector<EncoderLayerW> layers((size_t)L);
    const float *p = weights;
    for (EncoderLayerW &ly : layers) ly = pack_encoder_layer(pk, p, (size_t)d, (size_t)I, whisper, key_bias != 0);
    DevBuf tmp, w16, w32;
    PCE_TRY(upload_weights(c, pk, tmp, w16, w32));
    // the run's buffers, each holding what the caller's array of its first layer holds (a post-LN stack's r.ln: the caller's opening LayerNorm), and V^T zeroed once
    std::vector<int> tab((size_t)2 * n_items);
    for (int i = 0; i < n_items; i++) { tab[(size_t)i] = i * rows_per_item; tab[(size_t)n_items + i] = len[i]; }
    DevBuf dtab, dres, dln, dqk, dvt, dattn, dhid, cln, cqk, cvt, cattn, chid, cx;
    PCE_UPLOAD(c, dtab, tab);
    PCE_UPLOAD(c, dres, stream, (size_t)Md);
    PCE_UPLOAD(c, dln, pre ? ln16 : ln_in, (size_t)Md, 2048);
    PCE_UPLOAD(c, dqk, qk, (size_t)(2 * Md), 2048);
    PCE_UPLOAD(c, dattn, attn, (size_t)Md, 2048);
    PCE_UPLOAD(c, dhid, hidden, (size_t)MI, 2048);
    PCE_ZERO(op_t, c, dvt, (size_t)nvt + 64);
    // the captures: the caller's arrays, which keep their values where no launch writes
    PCE_UPLOAD(c, cln, ln16, (size_t)(L * 3 * Md)); PCE_UPLOAD(c, cqk, qk, (size_t)(L * 2 * Md)); PCE_UPLOAD(c, cvt, vt, (size_t)(L * nvt));
    PCE_UPLOAD(c, cattn, attn, (size_t)(L * Md)); PCE_UPLOAD(c, chid, hidden, (size_t)(L * MI)); PCE_UPLOAD(c, cx, x32, (size_t)(L * 4 * Md));
    const int *row0 = dtab.as<int>(), *lens = row0 + n_items;
    const double attn_flops = whisper ? 4.0 * rows_per_item * (double)rows_per_item * d * n_items : 0.0;
    const EncoderRun r{(int)M, d, heads, (int)I, n_items, rows_per_item, vt_sp, row0, lens, eps, attn_flops, whisper, dres.as<float>(), dln.as<op_t>(), dqk.as<op_t>(),
                       dvt.as<op_t>(), dattn.as<op_t>(), dhid.as<op_t>(), w16.as<op_t>(), w32.as<float>()};
    hipError_t copied = hipSuccess;
    const WalkCapture probe{c, &r, pre, cln.as<op_t>(), cqk.as<op_t>(), cvt.as<op_t>(), cattn.as<op_t>(), chid.as<op_t>(), cx.as<float>(), (size_t)Md, (size_t)MI,
                            (size_t)nvt, &copied};
    const bool fit = gemm_rule ? selftest_walk_w2v(c, r, layers, pre, probe) : encoder_walk<ProductGemm>(c, r, layers, pre, probe);
    PCE_HIP(c, hipGetLastError());
    PCE_HIP(c, copied);
    PCE_FETCH(c, ln16, cln.p, (size_t)(L * 3 * Md)); PCE_FETCH(c, qk, cqk.p, (size_t)(L * 2 * Md)); PCE_FETCH(c, vt, cvt.p, (size_t)(L * nvt));
    PCE_FETCH(c, attn, cattn.p, (size_t)(L * Md)); PCE_FETCH(c, hidden, chid.p, (size_t)(L * MI)); PCE_FETCH(c, x32, cx.p, (size_t)(L * 4 * Md));
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    if (fit_out) *fit_out = fit ? 1 : 0;
    return PCE_OK;
}

} // namespace PCE_BUILD_NS
