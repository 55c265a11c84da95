// pce_whisper_decoder.inc -- the Whisper text decoder's entry points (included by pce_whisper_impl.inc, whose kernels and launchers they use):
// weights, the prefix pass over padded token rows (forced alignment and the prefill of a decoding step share it), incremental steps, the device-resident loop,
// language detection (a decoding call's first half -- prompts to the last position's LayerNorm -- then the language rows of the output projection).
int pce_dtw_launch(pce_ctx *c, const double *d_x, int64_t x_stride, int ld, const int *d_rows, const int *d_cols, int N_max, int M_max,
                   int batch, unsigned char *d_trace, int *d_pi, int *d_pj, int *d_pl);

// Cross-attention keys (rows, [Ma][d]) and values (transposed per clip, key axis padded to AT_SP) of one decoder layer from the
// encoded audio: W = [K weights | V weights] (2d rows of d).  On the persistent 256 x 256 kernel when the shape fits.
static void project_cross_kv(pce_ctx *c, const op_t *enc, int Ma, int d, const op_t *W, const float *bias, op_t *xk, op_t *xvt)
{
    // one launch: K columns leave row-major, V columns as the transposed image (the 590 MB of encoded audio are swept once)
    if (launch_gemm_flat<FEPI_SPLIT>(c, enc, W, bias, xk, Ma, 2 * d, d, d, W_CTX, AT_SP, PCE_K_GEMM_FLAT_XKV, xvt, d)) return;
    launch_gemm<EPI_QKV>(c, enc, d, 0, W, Ma, 2 * d, d, bias, xk, d, 0, 1, reinterpret_cast<const float *>(xvt), W_CTX, d, AT_SP);
}

// ---- The prefix pass: the decoder over every position of padded token rows.  pce_whisper_align_run and the prefill of decode_step_device walk
// their layers through the functions below; their loops show what is their own (where V^T and the cross K / V live, the prefill's cache
// launches, the alignment's scores and the early end of its last layer).
constexpr int PREFIX_SP = 512;               // key pitch of the self-attention V^T images [clip][d][PREFIX_SP] (n_text_ctx <= 448)
// Token lists (lengths checked by the caller; `noun`: its word for an id in the error message) -> tok: one row of T_pad ids per sequence, zero padded;
// tab: per-clip tables [q_row0 | q_len | a_row0 | a_len | the caller's further columns], n entries each.  T_pad: the longest list rounded up to 16 (a V^T store writes 4
// positions, an MFMA row block is 16 rows): a step over the 3-token start sequence used to run 64 rows per clip (10.8 ms per 256 clips against 3.4 for an incremental step).
struct TokenRows { int T_pad = 0; std::vector<int> t_len, tok, tab; };
static int pad_token_rows(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, int n, int V, const char *noun, int columns, TokenRows &r)
{
    int T_max = 0; r.t_len.resize((size_t)n);
    for (int i = 0; i < n; i++) { r.t_len[(size_t)i] = token_offsets[i + 1] - token_offsets[i]; T_max = std::max(T_max, r.t_len[(size_t)i]); }
    r.T_pad = token_rows_pad(T_max);
    r.tok.assign((size_t)n * r.T_pad, 0); r.tab.assign((size_t)columns * n, 0);
    for (int i = 0; i < n; i++) {
        r.tab[(size_t)i] = i * r.T_pad; r.tab[(size_t)n + i] = r.t_len[(size_t)i];
        if (columns >= 4) { r.tab[(size_t)2 * n + i] = i * W_CTX; r.tab[(size_t)3 * n + i] = W_CTX; }
        for (int t = 0; t < r.t_len[(size_t)i]; t++) {
            const int v = tokens[token_offsets[i] + t];
            if (v < 0 || v >= V) return pce_fail(c, PCE_E_INVALID, "%s %d out of the vocabulary", noun, v);
            r.tok[(size_t)i * r.T_pad + t] = v;
        }
    }
    return PCE_OK;
}
// One run: Mt = n * T_pad rows of width d, H heads; the first four tables (uploaded to d_tab) and the decoder's weights
struct PrefixRun { int n, T_pad, d, H; int64_t Mt; const int *T0, *TL, *A0, *AL; const op_t *Wb; const float *Wf; };
static PrefixRun prefix_run(const WhisperState *w, int n, int T_pad)
{
    const int *T0 = w->d_tab.as<int>();
    return PrefixRun{n, T_pad, w->tdims.n_state, w->tdims.n_head, (int64_t)n * T_pad, T0, T0 + n, T0 + 2 * n, T0 + 3 * n, w->dw_bf16.as<op_t>(), w->dw_f32.as<float>()};
}
static int prefix_reserve_and_embed(pce_ctx *c, WhisperState *w, const PrefixRun &r)
{
    const size_t rows16 = sizeof(op_t) * (size_t)r.Mt * r.d;         // bytes of one op_t image of the rows
    PCE_HIP(c, w->d_resid.reserve(sizeof(float) * (size_t)r.Mt * r.d)); PCE_HIP(c, w->d_ln.reserve(rows16 + 4096));
    PCE_HIP(c, w->d_qk.reserve(2 * rows16 + 4096)); PCE_HIP(c, w->d_q.reserve(rows16 + 4096)); PCE_HIP(c, w->d_hidden.reserve(4 * rows16 + 4096));
    // k_attention writes the rows of real tokens only: the pad rows (T..T_pad of every clip) must not hold stale bits, a NaN
    // there would reach the next layer's V^T and poison valid queries through 0 * NaN (seen as an intermittent NaN cost matrix)
    PCE_ZERO(op_t, c, w->d_attn, (size_t)r.Mt * r.d + 2048);
    hipLaunchKernelGGL(k_embed_tokens, dim3((unsigned)div_up(r.Mt * r.d, 256)), dim3(256), 0, c->stream, w->d_tokens.as<int>(),
                       w->d_tok_emb.as<float>(), w->d_pos_emb.as<float>(), r.T_pad, w->tdims.n_text_ctx, r.d, r.Mt, w->d_resid.as<float>());
    return PCE_OK;
}
// LN -> Q | K rows into d_qk, V^T into the caller's image svt (the prefill copies K / V into its caches before the attention runs)
static void prefix_self_qkv(pce_ctx *c, WhisperState *w, const PrefixRun &r, const WhisperState::DLayer &ly, op_t *svt)
{
    launch_layernorm<op_t>(c, w->d_resid.as<float>(), r.Wf + ly.ln1_w, r.Wf + ly.ln1_b, r.Mt, r.d, w->d_ln.as<op_t>());
    launch_gemm<EPI_QKV>(c, w->d_ln.as<op_t>(), r.d, 0, r.Wb + ly.qkv_w, (int)r.Mt, 3 * r.d, r.d, r.Wf + ly.qkv_b, w->d_qk.as<op_t>(), 2 * r.d, 0, 1,
                         reinterpret_cast<const float *>(svt), r.T_pad, 2 * r.d, PREFIX_SP);
}
// masked self-attention -> output projection into the stream; LN -> the cross-attention queries into d_q
static void prefix_self_attention(pce_ctx *c, WhisperState *w, const PrefixRun &r, const WhisperState::DLayer &ly, const op_t *svt)
{
    launch_attention_rows(c, r.n, r.H, r.T_pad, w->d_qk.as<op_t>(), 2 * r.d, w->d_qk.as<op_t>() + r.d, 2 * r.d, svt, PREFIX_SP, r.T0, r.TL, r.T0, r.TL,
                          w->d_attn.as<op_t>(), 1);
    launch_gemm<EPI_RESID_F32>(c, w->d_attn.as<op_t>(), r.d, 0, r.Wb + ly.out_w, (int)r.Mt, r.d, r.d, r.Wf + ly.out_b, w->d_resid.as<float>(), r.d, 0, 1);
    launch_layernorm<op_t>(c, w->d_resid.as<float>(), r.Wf + ly.lnx_w, r.Wf + ly.lnx_b, r.Mt, r.d, w->d_ln.as<op_t>());
    launch_gemm<EPI_BF16>(c, w->d_ln.as<op_t>(), r.d, 0, r.Wb + ly.xq_w, (int)r.Mt, r.d, r.d, r.Wf + ly.xq_b, w->d_q.as<op_t>(), r.d, 0, 1);
}
// attention of d_q over the audio features (keys xk [n * 1500][d], values xvt [clip][d][AT_SP]) into d_attn (the alignment's scores follow it)
static void prefix_cross_attention(pce_ctx *c, WhisperState *w, const PrefixRun &r, const op_t *xk, const op_t *xvt)
{
    launch_attention_rows(c, r.n, r.H, r.T_pad, w->d_q.as<op_t>(), r.d, xk, r.d, xvt, AT_SP, r.T0, r.TL, r.A0, r.AL, w->d_attn.as<op_t>(), 0);
}
// cross-attention output projection; LN -> fc1 + GELU -> fc2.  fc1_persistent: fc1 on the persistent 256 x 256 kernel when the width allows it -- by the model's dims alone,
// like every kernel (12 column tiles x 36 row tiles at Whisper-small size: 91 -> ~55 us per launch, and fc2 behind it reads a warmer cache; profiles/r05/align_fc1_flat_ab.txt)
static void prefix_cross_out_mlp(pce_ctx *c, WhisperState *w, const PrefixRun &r, const WhisperState::DLayer &ly, bool fc1_persistent)
{
    const op_t *ln = w->d_ln.as<op_t>(), *W1 = r.Wb + ly.m1_w;
    launch_gemm<EPI_RESID_F32>(c, w->d_attn.as<op_t>(), r.d, 0, r.Wb + ly.xout_w, (int)r.Mt, r.d, r.d, r.Wf + ly.xout_b, w->d_resid.as<float>(), r.d, 0, 1);
    launch_layernorm<op_t>(c, w->d_resid.as<float>(), r.Wf + ly.ln2_w, r.Wf + ly.ln2_b, r.Mt, r.d, w->d_ln.as<op_t>());
    if (!fc1_persistent || !launch_gemm_flat<FEPI_GELU>(c, ln, W1, r.Wf + ly.m1_b, w->d_hidden.as<op_t>(), (int)r.Mt, 4 * r.d, r.d, 4 * r.d, 1, 0, PCE_K_GEMM_FLAT_FC1))
        launch_gemm<EPI_GELU_BF16>(c, ln, r.d, 0, W1, (int)r.Mt, 4 * r.d, r.d, r.Wf + ly.m1_b, w->d_hidden.as<op_t>(), 4 * r.d, 0, 1);
    launch_gemm<EPI_RESID_F32>(c, w->d_hidden.as<op_t>(), 4 * r.d, 0, r.Wb + ly.m2_w, (int)r.Mt, r.d, 4 * r.d, r.Wf + ly.m2_b, w->d_resid.as<float>(), r.d, 0, 1);
}

namespace PCE_BUILD_NS {

int pce_whisper_decoder_load(pce_ctx *c, const pce_whisper_text_dims *dims, const float *weights, int64_t n_floats)
{
    if (!c || !dims || !weights) return PCE_E_INVALID;
    const int d = dims->n_state, L = dims->n_layer, V = dims->n_vocab, TC = dims->n_text_ctx;
    if (d <= 0 || d % 128 || dims->n_head * 64 != d || L <= 0 || V <= 0 || V > DR_K * DR_T || TC <= 0 || TC > 448)
        return pce_fail(c, PCE_E_LIMIT, "unsupported decoder dims (need n_state %% 128 == 0, head size 64, n_text_ctx <= 448, n_vocab <= 52224)");
    if (dims->n_head > 32) return pce_fail(c, PCE_E_LIMIT, "decoder with %d heads: the decoding kernels take at most 32", dims->n_head);
    static_assert(32 * 64 <= LN_D_MAX, "the decoder's LayerNorms must hold 32 heads");
    const int64_t per_layer = 2LL * d + (4LL * d * d + 3LL * d) + 2LL * d + (4LL * d * d + 3LL * d) + 2LL * d + 8LL * d * d + 5LL * d;
    const int64_t expect = (int64_t)V * d + (int64_t)TC * d + L * per_layer + 2LL * d;
    if (n_floats != expect) return pce_fail(c, PCE_E_INVALID, "decoder weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)expect);
    PCE_HIP(c, hipSetDevice(c->device));
    WhisperState *w = ws_of(c);
    PCE_TRY(lds_optins(c, w));
    w->tdims = *dims; w->dec_loaded = false; w->dlayers.assign((size_t)L, {});
    WeightPack pk;
    const float *p = weights;
    const float *tok = p; p += (size_t)V * d;
    const float *pos = p; p += (size_t)TC * d;
    const size_t dd = (size_t)d * d;
    for (WhisperState::DLayer &ly : w->dlayers) {
        ly.ln1_w = pk.vec(p, (size_t)d); ly.ln1_b = pk.vec(p, (size_t)d);
        { const WeightPack::Attn a = pk.self_attention(p, (size_t)d, false); ly.qkv_w = a.qkv_w; ly.qkv_b = a.qkv_b; ly.out_w = a.out_w; ly.out_b = a.out_b; }
        ly.lnx_w = pk.vec(p, (size_t)d); ly.lnx_b = pk.vec(p, (size_t)d);
        // cross attention: q from text, k | v from audio -> [d][d] and fused [2d][d] with bias [0 | v.b]
        ly.xq_w = pk.mat(p, dd); ly.xq_b = pk.vec(p, (size_t)d);
        ly.xkv_w = pk.mat(p, dd); pk.mat(p, dd);
        ly.xkv_b = pk.zeros((size_t)d); pk.vec(p, (size_t)d);
        ly.xout_w = pk.mat(p, dd); ly.xout_b = pk.vec(p, (size_t)d);
        ly.ln2_w = pk.vec(p, (size_t)d); ly.ln2_b = pk.vec(p, (size_t)d);
        ly.m1_w = pk.mat(p, 4 * dd); ly.m1_b = pk.vec(p, (size_t)4 * d);
        ly.m2_w = pk.mat(p, 4 * dd); ly.m2_b = pk.vec(p, (size_t)d);
    }
    w->dln_w = pk.vec(p, (size_t)d); w->dln_b = pk.vec(p, (size_t)d);
    DevBuf tmp;
    PCE_TRY(upload_weights(c, pk, tmp, w->dw_bf16, w->dw_f32));
    PCE_UPLOAD(c, w->d_tok_emb, tok, (size_t)V * d);
    PCE_UPLOAD(c, w->d_pos_emb, pos, (size_t)TC * d);
    {   // tied output projection for free-running decoding: the token embedding in op_t, rows padded to the 128-column GEMM tile
        const size_t Vp = (size_t)div_up(V, 128) * 128;
        PCE_ZERO(op_t, c, w->g_emb_bf16, Vp * (size_t)d, 128);
        hipLaunchKernelGGL(k_f32_to_bf16, dim3((unsigned)div_up((int64_t)V * d, 256)), dim3(256), 0, c->stream, w->d_tok_emb.as<float>(),
                           w->g_emb_bf16.as<op_t>(), (int64_t)V * d);
    }
    {   // Wk^T of every layer's cross-attention: the second operand of k_xq_fused (pce_xattn.inc)
        PCE_HIP(c, w->g_wkT.reserve(sizeof(op_t) * dd * (size_t)L + 256));
        for (int l = 0; l < L; l++)
            hipLaunchKernelGGL(k_transpose_sq, dim3((unsigned)(d / 32), (unsigned)(d / 32)), dim3(256), 0, c->stream, w->dw_bf16.as<op_t>() + w->dlayers[(size_t)l].xkv_w,
                               w->g_wkT.as<op_t>() + dd * (size_t)l, d);
    }
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    w->dec_loaded = true; w->g_xkv_clips = -1; w->g_cache_len = -1;
    w->g_cache_n = -1;                  // the self-attention cache is sized by THIS decoder's width and layers: another decoder, another cache
    return PCE_OK;
}

int pce_whisper_align_run(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const int32_t *num_frames, int32_t sot_len,
                          const uint8_t *head_mask, int32_t medfilt_width, float qk_scale)
{
    if (!c || !tokens || !token_offsets || !num_frames) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (!w->dec_loaded) return pce_fail(c, PCE_E_STATE, "pce_whisper_align_run before pce_whisper_decoder_load");
    if (w->n_clips_enc < 0) return pce_fail(c, PCE_E_STATE, "run pce_whisper_encode_run first");
    if (w->tdims.n_state != w->dims.n_state) return pce_fail(c, PCE_E_INVALID, "decoder and encoder widths differ");
    if (!align_width_ok(medfilt_width)) return pce_fail(c, PCE_E_INVALID, "median filter width must be odd, <= 15");
    PCE_HIP(c, hipSetDevice(c->device));
    const int n = w->n_clips_enc, d = w->tdims.n_state, H = w->tdims.n_head, L = w->tdims.n_layer, V = w->tdims.n_vocab;
    // ---- shapes
    AlignDims dims;
    std::vector<int> f_len((size_t)n);
    for (int i = 0; i < n; i++) {
        const int F = std::min(num_frames[i] / 2, W_CTX);
        PCE_TRY(align_clip_dims(c, i, token_offsets[i + 1] - token_offsets[i], F, sot_len, w->tdims.n_text_ctx, dims));
        f_len[(size_t)i] = F;
    }
    const int F_max = dims.F_max, N_max = dims.N_max, F_pad = dims.F_pad();
    const int64_t Ma = (int64_t)n * W_CTX;
    // selected heads (default: every head of the last half of the layers, as whisper's Whisper.__init__ sets alignment_heads)
    std::vector<int> heads; std::vector<int> layer_first((size_t)L + 1, 0);
    for (int l = 0; l < L; l++) {
        layer_first[(size_t)l] = (int)heads.size();
        for (int hh = 0; hh < H; hh++)
            if (head_mask ? head_mask[l * H + hh] != 0 : l >= L / 2) heads.push_back(hh);
    }
    layer_first[(size_t)L] = (int)heads.size();
    const int n_sel = (int)heads.size();
    if (n_sel == 0) return pce_fail(c, PCE_E_INVALID, "no alignment head selected");
    // ---- tables: [q_row0 | q_len | a_row0 | a_len | f_len | n_rows(dtw)] and padded tokens
    TokenRows rows;
    PCE_TRY(pad_token_rows(c, tokens, token_offsets, n, V, "token", 6, rows));
    const int T_pad = rows.T_pad;
    std::vector<int> &tab = rows.tab, &tok = rows.tok;
    for (int i = 0; i < n; i++) { tab[(size_t)4 * n + i] = f_len[(size_t)i]; tab[(size_t)5 * n + i] = rows.t_len[(size_t)i] - sot_len - 1; }
    w->al_rows.assign(tab.begin() + 5 * n, tab.begin() + 6 * n); w->al_cols = f_len;
    {
        const size_t c0 = w->d_tab.cap, c1 = w->d_tokens.cap, c2 = w->d_heads.cap;
        PCE_HIP(c, w->d_tab.reserve(sizeof(int) * tab.size()));
        PCE_HIP(c, w->d_tokens.reserve(sizeof(int) * tok.size()));
        PCE_HIP(c, w->d_heads.reserve(sizeof(int) * heads.size()));
        if (c0 != w->d_tab.cap || c1 != w->d_tokens.cap || c2 != w->d_heads.cap) w->al_tab_host.clear();     // reallocated: nothing is held
    }
    // the tables go up (and the host waits for the copy out of these pageable vectors: a drain of everything queued before, the encoder
    // included) only when they differ from what the device already holds: a caller that aligns the same token lists again -- the
    // bench's step, a retried batch -- keeps enqueuing
    if (w->al_tab_host.empty() || tab != w->al_tab_host || tok != w->al_tok_host || heads != w->al_heads_host) {
        PCE_PUT(c, w->d_tab.p, tab.data(), tab.size());
        PCE_PUT(c, w->d_tokens.p, tok.data(), tok.size());
        PCE_PUT(c, w->d_heads.p, heads.data(), heads.size());
        PCE_HIP(c, hipStreamSynchronize(c->stream));
        w->al_tab_host = tab; w->al_tok_host = tok; w->al_heads_host = heads;
    }
    const PrefixRun run = prefix_run(w, n, T_pad);
    const int *TL = run.TL, *FL = run.T0 + 4 * n, *NR = run.T0 + 5 * n;
    // ---- buffers (those of the prefix pass itself: prefix_reserve_and_embed)
    PCE_HIP(c, w->d_enc_bf16.reserve(sizeof(op_t) * (size_t)Ma * d + 4096));
    PCE_HIP(c, w->d_vt.reserve(sizeof(op_t) * ((size_t)n * (size_t)d * PREFIX_SP + 64)));
    if (w->d_vt.cap != w->dvt_zero_cap) {                     // (only ever holds finite values afterwards: columns past a sequence's tokens are masked, never NaN)
        PCE_HIP(c, hipMemsetAsync(w->d_vt.p, 0, w->d_vt.cap, c->stream));
        w->dvt_zero_cap = w->d_vt.cap;
    }
    PCE_HIP(c, w->d_aw.reserve(sizeof(float) * (size_t)n * n_sel * T_pad * (size_t)F_pad));
    PCE_HIP(c, w->d_cost.reserve(sizeof(double) * (size_t)n * N_max * (size_t)F_pad));
    PCE_HIP(c, w->d_trace.reserve((size_t)n * (size_t)(N_max + 1) * (size_t)(F_max + 1)));
    PCE_HIP(c, w->d_pi.reserve(sizeof(int) * (size_t)n * (size_t)(N_max + F_max)));
    PCE_HIP(c, w->d_pj.reserve(sizeof(int) * (size_t)n * (size_t)(N_max + F_max)));
    PCE_HIP(c, w->d_pl.reserve(sizeof(int) * (size_t)n));
    // the audio keys/values reuse the encoder's q|k and V^T buffers (the encoder is finished)
    op_t *xk = w->qkv.as<op_t>(), *xvt = w->vt.as<op_t>();
    // when a decoding step has already projected this encoded batch (pce_whisper_decode_step keeps the cross K / V of all
    // layers), the 12 projections (15 of this call's 27 ms at 256 clips) are read from there
    const bool xkv_cached = w->g_xkv_clips == n;
    const size_t xk_cl = (size_t)Ma * d, xvt_cl = (size_t)n * (size_t)d * AT_SP;
    const AlignMatrix am{w->d_aw.as<float>(), TL, FL, n, n_sel, T_pad, F_pad};
    KernelTimer timer(c, PCE_K_WHISPER_ALIGN);
    if (w->enc_bf16_clips != n)                                   // (the persistent-GEMM encoder path has already written it)
        hipLaunchKernelGGL(k_f32_to_bf16, dim3((unsigned)div_up(Ma * d, 256)), dim3(256), 0, c->stream, w->final_out.as<float>(),
                               w->d_enc_bf16.as<op_t>(), Ma * d);
    PCE_TRY(prefix_reserve_and_embed(c, w, run));
    for (int l = 0; l < L; l++) {
        const WhisperState::DLayer &ly = w->dlayers[(size_t)l];
        prefix_self_qkv(c, w, run, ly, w->d_vt.as<op_t>());
        prefix_self_attention(c, w, run, ly, w->d_vt.as<op_t>());
        if (xkv_cached) { xk = w->g_xk.as<op_t>() + xk_cl * (size_t)l; xvt = w->g_xvt.as<op_t>() + xvt_cl * (size_t)l; }
        else if (l + 1 < L || !launch_gemm_flat<FEPI_BF16>(c, w->d_enc_bf16.as<op_t>(), run.Wb + ly.xkv_w, run.Wf + ly.xkv_b, xk, (int)Ma, d, d, d, 1, 0, PCE_K_GEMM_FLAT_XKV))
            project_cross_kv(c, w->d_enc_bf16.as<op_t>(), (int)Ma, d, run.Wb + ly.xkv_w, run.Wf + ly.xkv_b, xk, xvt);      // (the last layer: keys only when the 256 x 256 kernel takes the shape -- its values are never read, see below)
        // Nothing downstream reads the decoder's output here (find_alignment's token probabilities are not produced by this entry point: the
        // alignment matrix is all that leaves), so the last layer ends at its alignment scores: its cross-attention product, output projection
        // and MLP are not run (round 5)
        const bool tail = l + 1 < L;
        if (tail) prefix_cross_attention(c, w, run, xk, xvt);
        const int ns_l = layer_first[(size_t)l + 1] - layer_first[(size_t)l];
        if (ns_l > 0) launch_align_scores(c, am, w->d_q.as<op_t>(), xk, d, w->d_heads.as<int>(), layer_first[(size_t)l], ns_l, qk_scale);
        if (!tail) break;
        prefix_cross_out_mlp(c, w, run, ly, true);
    }
    // alignment matrix: normalise over tokens, median filter over time, mean over heads, DTW
    launch_align_cost(c, am, (int)sot_len, (int)medfilt_width, N_max, w->d_cost.as<double>());
    PCE_TRY(pce_dtw_launch(c, w->d_cost.as<double>(), (int64_t)N_max * F_pad, F_pad, NR, FL, N_max, F_max, n, w->d_trace.as<unsigned char>(),
                           w->d_pi.as<int>(), w->d_pj.as<int>(), w->d_pl.as<int>()));
    PCE_HIP(c, hipGetLastError());
    w->al_n = n; w->al_Nmax = N_max; w->al_Fpad = F_pad; w->al_Mmax = F_max;
    return PCE_OK;
}

int pce_whisper_align_fetch(pce_ctx *c, int32_t clip, int32_t *text_idx, int32_t *time_idx, int32_t *path_len, double *cost)
{
    if (!c || !path_len) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (w->al_n < 0) return pce_fail(c, PCE_E_STATE, "pce_whisper_align_fetch before pce_whisper_align_run");
    if (clip < 0 || clip >= w->al_n) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    PCE_HIP(c, hipSetDevice(c->device));
    const size_t stride = (size_t)(w->al_Nmax + w->al_Mmax);
    int n = 0;
    PCE_FETCH(c, &n, w->d_pl.as<int>() + clip, 1);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    *path_len = n;
    if (text_idx) PCE_FETCH(c, text_idx, w->d_pi.as<int>() + stride * (size_t)clip, (size_t)n);
    if (time_idx) PCE_FETCH(c, time_idx, w->d_pj.as<int>() + stride * (size_t)clip, (size_t)n);
    if (cost) {
        const int N = w->al_rows[(size_t)clip], F = w->al_cols[(size_t)clip];
        PCE_HIP(c, hipMemcpy2DAsync(cost, sizeof(double) * (size_t)F, w->d_cost.as<double>() + (size_t)clip * w->al_Nmax * (size_t)w->al_Fpad,
                                    sizeof(double) * (size_t)w->al_Fpad, sizeof(double) * (size_t)F, (size_t)N, hipMemcpyDeviceToHost, c->stream));
    }
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

int pce_whisper_align_paths_enqueue(pce_ctx *c, int32_t slot, int32_t *n_clips, int32_t *path_stride)
{
    if (!c || slot < 0 || slot > 1) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (w->al_n < 0) return pce_fail(c, PCE_E_STATE, "pce_whisper_align_paths_enqueue before pce_whisper_align_run");
    PCE_HIP(c, hipSetDevice(c->device));
    WhisperState::PathSlot &ps = w->al_slot[slot];
    // a slot whose previous fetch nobody has waited for: its copies may still be in flight into the pinned buffer this call would overwrite (or free and
    // reallocate, if the new batch is larger) -- the caller's protocol error (ADVICE r05), reported instead of raced
    if (ps.armed) return pce_fail(c, PCE_E_STATE, "pce_whisper_align_paths_enqueue: slot %d still holds an enqueued fetch (pce_whisper_align_paths_wait first)", slot);
    const size_t n = (size_t)w->al_n, stride = (size_t)(w->al_Nmax + w->al_Mmax), ints = n * (2 * stride + 1);
    if (sizeof(int) * ints > ps.cap) {
        if (ps.host) { PCE_HIP(c, hipHostFree(ps.host)); ps.host = nullptr; ps.cap = 0; }
        PCE_HIP(c, hipHostMalloc(&ps.host, sizeof(int) * ints + (sizeof(int) * ints >> 2), hipHostMallocDefault));
        ps.cap = sizeof(int) * ints + (sizeof(int) * ints >> 2);
    }
    if (!ps.ev) PCE_HIP(c, hipEventCreateWithFlags(&ps.ev, hipEventDisableTiming));
    int *h = static_cast<int *>(ps.host);
    // behind the DTW on the context's stream: lengths, then the two index arrays as they lie ([clip][stride], a few MB at most)
    PCE_FETCH(c, h, w->d_pl.p, n);
    PCE_FETCH(c, h + n, w->d_pi.p, n * stride);
    PCE_FETCH(c, h + n + n * stride, w->d_pj.p, n * stride);
    PCE_HIP(c, hipEventRecord(ps.ev, c->stream));
    ps.armed = true; ps.n = (int)n; ps.stride = (int)stride;
    if (n_clips) *n_clips = (int32_t)n;
    if (path_stride) *path_stride = (int32_t)stride;
    return PCE_OK;
}

int pce_whisper_align_paths_wait(pce_ctx *c, int32_t slot, int32_t *path_len, int32_t *text_idx, int32_t *time_idx)
{
    if (!c || slot < 0 || slot > 1 || !path_len) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    WhisperState::PathSlot &ps = w->al_slot[slot];
    if (!ps.armed) return pce_fail(c, PCE_E_STATE, "pce_whisper_align_paths_wait: slot %d has no enqueued fetch", slot);
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_HIP(c, hipEventSynchronize(ps.ev));
    ps.armed = false;
    const int *h = static_cast<const int *>(ps.host);
    const size_t n = (size_t)ps.n, stride = (size_t)ps.stride;
    memcpy(path_len, h, sizeof(int) * n);
    for (size_t i = 0; i < n; i++) {
        const size_t len = (size_t)(h[i] < 0 ? 0 : h[i]);
        if (len > stride) return pce_fail(c, PCE_E_STATE, "clip %zu: a DTW path of %zu steps in a buffer of %zu", i, len, stride);
        if (text_idx) memcpy(text_idx + i * stride, h + n + i * stride, sizeof(int) * len);
        if (time_idx) memcpy(time_idx + i * stride, h + n + n * stride + i * stride, sizeof(int) * len);
    }
    return PCE_OK;
}

int pce_whisper_align_shape(pce_ctx *c, int32_t clip, int32_t *n_rows, int32_t *n_cols)
{
    if (!c) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (w->al_n < 0) return pce_fail(c, PCE_E_STATE, "pce_whisper_align_shape before pce_whisper_align_run");
    if (clip < 0 || clip >= w->al_n) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    if (n_rows) *n_rows = w->al_rows[(size_t)clip];
    if (n_cols) *n_cols = w->al_cols[(size_t)clip];
    return PCE_OK;
}

// ---------------------------------------------------------------------------
// Free-running decoding, one step: the text decoder over the sequences so far (cross K / V of every layer computed once
// per encoded batch and kept; a prefix pass fills the self-attention K / V cache, a step that extends it by one token
// runs that position alone), logits of the last position through the tied output projection, openai-whisper's logit
// filters and greedy choice.  The loop over steps, the prompt and the stopping rule are host logic (Aligners/decoding.py).
// ---------------------------------------------------------------------------
int pce_whisper_decode_step(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, int32_t sample_begin,
                                       const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, int32_t *next_tokens,
                                       float *next_logprobs)
{
    pce_whisper_decode_opts o{};
    o.sample_begin = nullptr; o.sample_begin_all = sample_begin; o.temperature = 0.f; o.probe_token = -1;
    return PCE_BUILD_NS::pce_whisper_decode_step_ex(c, tokens, token_offsets, rules, vocab_mask, &o, next_tokens, next_logprobs, nullptr);
}

// launches of ONE incremental step (one new position per sequence) from the tables ct[8 n] (see k_step_advance) -- host-uploaded by
// pce_whisper_decode_step_ex, device-maintained inside pce_whisper_decode_loop -- down to the final LayerNorm of the new position
static void decode_incremental_launches(pce_ctx *c, WhisperState *w, int n, const int *CT, const int *ended)
{
    const int d = w->tdims.n_state, H = w->tdims.n_head, L = w->tdims.n_layer, SPD = 512, T_cap = w->tdims.n_text_ctx;
    const int64_t Ma = (int64_t)n * W_CTX;
    const size_t xk_l = (size_t)Ma * d, xvt_l = (size_t)n * (size_t)d * AT_SP, sk_l = (size_t)n * T_cap * d, svt_l = (size_t)n * (size_t)d * SPD;
    const op_t *Wb = w->dw_bf16.as<op_t>();
    const float *Wf = w->dw_f32.as<float>();
    const int *K0 = CT + 3 * n, *KL = CT + 4 * n, *X0 = CT + 5 * n, *XL = CT + 6 * n, *POS = CT + 7 * n;
    struct FewRows { pce_ctx *c; explicit FewRows(pce_ctx *cc) : c(cc) { c->gemm_few_rows = true; } ~FewRows() { c->gemm_few_rows = false; } } few_rows(c);
    hipLaunchKernelGGL(k_embed_one, dim3((unsigned)div_up((int64_t)n * d, 256)), dim3(256), 0, c->stream, CT, w->d_tok_emb.as<float>(),
                       w->d_pos_emb.as<float>(), POS, d, n, w->g_c_resid.as<float>());
    // the self-attention kernel also appends the new position to its cache
    auto cattn = [&](const op_t *q, int64_t q_ld, const op_t *k, int64_t k_ld, const op_t *vt, int64_t vt_clip, int vt_sp, const int *k0, const int *kl,
                     const op_t *app_qkv = nullptr) {
        // the streaming single-query kernels (the MFMA attention kernel would spend a 32-query tile on the one live query)
        Attn1Args a{};
        a.q = q; a.q_ld = q_ld; a.k = k; a.k_ld = k_ld; a.vt = vt; a.vt_clip = vt_clip; a.vt_sp = vt_sp; a.k_row0 = k0; a.k_len = kl; a.skip = ended;
        a.out = w->g_c_attn.as<op_t>(); a.out_ld = d;
        if (app_qkv) { a.app_k = app_qkv + d; a.app_v = app_qkv + 2 * d; a.app_ld = 3 * d; a.app_pos = POS; }
        launch_cross_attn1(c, n, H, a);
    };
    auto cln = [&](size_t w_off, size_t b_off) {
        launch_layernorm<op_t>(c, w->g_c_resid.as<float>(), Wf + w_off, Wf + b_off, (int64_t)n, d, w->g_c_ln.as<op_t>());
    };
    // cross-attention from the encoder output (pce_xattn.inc): E once per layer instead of K and V^T
    const bool absorb = c->sw.xattn_absorb && xa_has_form(d, H) && w->g_qp.p && w->g_wkT.p;
    static const int env_wpc = getenv("PCE_XATTN_WPC") ? atoi(getenv("PCE_XATTN_WPC")) : 0;
    XaArgs xa{};
    xa.E = w->d_enc_bf16.as<op_t>(); xa.e_clip = (int64_t)W_CTX * d; xa.e_ld = d; xa.k_len = XL; xa.skip = ended;
    xa.u_part = w->g_upart.as<float>(); xa.ml_part = w->g_mlpart.as<float>(); xa.heads = H; xa.nsplit = xa_split(n, env_wpc); xa.rows = xa_rows(H);
    auto xattn = [&](int l) {
        const WhisperState::DLayer &ly = w->dlayers[(size_t)l];
        XaLayer y{};
        y.resid = w->g_c_resid.as<float>(); y.ln_w = Wf + ly.lnx_w; y.ln_b = Wf + ly.lnx_b; y.wq = Wb + ly.xq_w; y.bq = Wf + ly.xq_b;
        y.wkT = w->g_wkT.as<op_t>() + (size_t)d * d * (size_t)l; y.wv = Wb + ly.xkv_w + (size_t)d * d; y.bv = Wf + ly.xkv_b + d;
        y.qp_hi = w->g_qp.as<op_t>(); y.qp_lo = y.qp_hi + (size_t)n * xa.rows * d; y.out = w->g_c_attn.as<op_t>(); y.out_ld = d;
        KernelTimer kt(c, PCE_K_CROSS_ATTN1);
        xattn_launch(c, d, n, xa, y);
    };
    for (int l = 0; l < L; l++) {
        const WhisperState::DLayer &ly = w->dlayers[(size_t)l];
        // (the LayerNorm as a prologue of the projection that consumes it -- every workgroup normalising its own 64 rows -- was measured
        //  and dropped: four dependent L2 round trips per wave, 17 us per launch against 11.8 + 5.5 for the two launches)
        cln(ly.ln1_w, ly.ln1_b);
        launch_gemm<EPI_BF16>(c, w->g_c_ln.as<op_t>(), d, 0, Wb + ly.qkv_w, n, 3 * d, d, Wf + ly.qkv_b, w->g_c_qkv.as<op_t>(), 3 * d, 0, 1);
        if (c->sw.self_rows && w->g_sv.p) {
            // row-major K / V caches: the append is two coalesced row stores (the V^T image is not touched by incremental steps: only prefix runs,
            // which rewrite every position they attend to, read it)
            SelfAttn1Args sa{};
            sa.qkv = w->g_c_qkv.as<op_t>(); sa.qkv_ld = 3 * d; sa.ck = w->g_sk.as<op_t>() + sk_l * (size_t)l; sa.cv = w->g_sv.as<op_t>() + sk_l * (size_t)l;
            sa.c_clip = (int64_t)T_cap * d; sa.d = d; sa.pos = POS; sa.skip = ended; sa.out = w->g_c_attn.as<op_t>(); sa.out_ld = d;
            launch_self_attn1(c, n, H, sa);
        } else
        cattn(w->g_c_qkv.as<op_t>(), 3 * d, w->g_sk.as<op_t>() + sk_l * (size_t)l, d, w->g_svt.as<op_t>() + svt_l * (size_t)l, (int64_t)d * SPD, SPD, K0, KL,
              w->g_c_qkv.as<op_t>());
        launch_gemm<EPI_RESID_F32>(c, w->g_c_attn.as<op_t>(), d, 0, Wb + ly.out_w, n, d, d, Wf + ly.out_b, w->g_c_resid.as<float>(), d, 0, 1);
        if (!absorb) cln(ly.lnx_w, ly.lnx_b);                       // (the encoder-output form normalises inside its first launch)
        if (!absorb) launch_gemm<EPI_BF16>(c, w->g_c_ln.as<op_t>(), d, 0, Wb + ly.xq_w, n, d, d, Wf + ly.xq_b, w->g_c_q.as<op_t>(), d, 0, 1);
        if (absorb) xattn(l);          // (its first launch is the query projection itself)
        else cattn(w->g_c_q.as<op_t>(), d, w->g_xk.as<op_t>() + xk_l * (size_t)l, d, w->g_xvt.as<op_t>() + xvt_l * (size_t)l, (int64_t)d * AT_SP, AT_SP, X0, XL);
        launch_gemm<EPI_RESID_F32>(c, w->g_c_attn.as<op_t>(), d, 0, Wb + ly.xout_w, n, d, d, Wf + ly.xout_b, w->g_c_resid.as<float>(), d, 0, 1);
        cln(ly.ln2_w, ly.ln2_b);
        launch_gemm<EPI_GELU_BF16>(c, w->g_c_ln.as<op_t>(), d, 0, Wb + ly.m1_w, n, 4 * d, d, Wf + ly.m1_b, w->g_c_hidden.as<op_t>(), 4 * d, 0, 1);
        launch_gemm<EPI_RESID_F32>(c, w->g_c_hidden.as<op_t>(), 4 * d, 0, Wb + ly.m2_w, n, d, 4 * d, Wf + ly.m2_b, w->g_c_resid.as<float>(), d, 0, 1);
    }
    launch_layernorm<op_t>(c, w->g_c_resid.as<float>(), Wf + w->dln_w, Wf + w->dln_b, (int64_t)n, d, w->g_lastln.as<op_t>());
}
static int decode_incremental_reserve(pce_ctx *c, WhisperState *w, int n)
{
    const int d = w->tdims.n_state;
    PCE_HIP(c, w->g_c_tab.reserve(sizeof(int) * 8 * (size_t)n));
    PCE_HIP(c, w->g_c_resid.reserve(sizeof(float) * (size_t)n * d));
    PCE_HIP(c, w->g_c_ln.reserve(sizeof(op_t) * (size_t)(n + 128) * d + 4096));
    PCE_HIP(c, w->g_c_qkv.reserve(sizeof(op_t) * (size_t)(n + 128) * 3 * d + 4096));
    {
        const size_t before = w->g_c_attn.cap;
        PCE_HIP(c, w->g_c_attn.reserve(sizeof(op_t) * (size_t)(n + 128) * d + 4096));
        if (w->g_c_attn.cap != before) PCE_HIP(c, hipMemsetAsync(w->g_c_attn.p, 0, w->g_c_attn.cap, c->stream));   // rows of ended sequences are skipped: never uninitialised bits
    }
    PCE_HIP(c, w->g_c_q.reserve(sizeof(op_t) * (size_t)(n + 128) * d + 4096));
    PCE_HIP(c, w->g_c_hidden.reserve(sizeof(op_t) * (size_t)(n + 128) * 4 * d + 4096));
    if (c->sw.xattn_absorb) {
        const size_t before = w->g_qp.cap, R = (size_t)xa_rows(w->tdims.n_head);   // R rows of heads per clip (pce_xattn.inc)
        PCE_HIP(c, w->g_qp.reserve(sizeof(op_t) * 2 * (size_t)n * R * d + 256));
        if (w->g_qp.cap != before) PCE_HIP(c, hipMemsetAsync(w->g_qp.p, 0, w->g_qp.cap, c->stream));               // (rows >= heads feed MFMA rows nobody reads: finite all the same)
        PCE_HIP(c, w->g_upart.reserve(sizeof(float) * (size_t)n * XA_MAX_SPLIT * R * d + 256));
        PCE_HIP(c, w->g_mlpart.reserve(sizeof(float) * (size_t)n * XA_MAX_SPLIT * R * 2 + 256));
    }
    return PCE_OK;
}

// one decoding step; results stay on the device in g_next (next token | log-probability | probe probability, n each).  `resident`: the
// caller (pce_whisper_decode_loop) keeps the tables of an incremental step on the device: `tokens` is then only consulted for step 0.
static int decode_step_device(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules,
                              const uint8_t *vocab_mask, const pce_whisper_decode_opts *opts, bool want_probe);

// the ids temperature sampling keys its noise by, one per clip of the encoded batch; they last until the next pce_whisper_encode_run
int pce_whisper_sample_keys(pce_ctx *c, const int32_t *keys, int32_t n)
{
    if (!c || n < 0 || (n > 0 && !keys)) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (n == 0) { w->g_keys_n = 0; return PCE_OK; }
    if (w->n_clips_enc < 0) return pce_fail(c, PCE_E_STATE, "pce_whisper_sample_keys before pce_whisper_encode_run");
    if (n != w->n_clips_enc) return pce_fail(c, PCE_E_INVALID, "pce_whisper_sample_keys: %d keys for %d encoded clips", n, w->n_clips_enc);
    PCE_HIP(c, hipSetDevice(c->device));
    // (pageable source: the copy has left `keys` when the call returns; it is ordered before the next decode on the same stream)
    PCE_UPLOAD(c, w->g_keys, keys, (size_t)n);
    w->g_keys_n = n;
    return PCE_OK;
}

int pce_whisper_decode_step_ex(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules,
                                          const uint8_t *vocab_mask, const pce_whisper_decode_opts *opts, int32_t *next_tokens,
                                          float *next_logprobs, float *probe_prob)
{
    if (!c || !tokens || !token_offsets || !rules || !vocab_mask || !next_tokens || !opts) return PCE_E_INVALID;
    PCE_TRY(decode_step_device(c, tokens, token_offsets, rules, vocab_mask, opts, probe_prob != nullptr));
    WhisperState *w = ws_of(c);
    const int n = w->n_clips_enc;
    if (n == 0) return PCE_OK;
    PCE_FETCH(c, next_tokens, w->g_next.p, (size_t)n);
    if (next_logprobs) PCE_FETCH(c, next_logprobs, w->g_next.as<int>() + n, (size_t)n);
    if (probe_prob && opts->probe_token >= 0)
        PCE_FETCH(c, probe_prob, w->g_next.as<int>() + 2 * n, (size_t)n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

// ---- A decoding call up to the final LayerNorm of every sequence's last position, in two parts (pce_whisper_decode_step_ex / pce_whisper_decode_loop go on to the
// output projection and the logit filters, pce_whisper_detect_language to the language rows of the embedding alone).
// Part 1, before the first launch: lengths checked against the text context, the prompts as padded token rows and the tables
// [q_row0 | q_len | a_row0 | a_len | sample_begin] on the device (with the vocabulary mask, when the caller has one), one synchronisation.
static int decode_stage_prompts(pce_ctx *c, WhisperState *w, const int32_t *tokens, const int32_t *token_offsets, const int32_t *sample_begin_of,
                                int32_t sample_begin_all, const uint8_t *vocab_mask, TokenRows &rows)
{
    const int n = w->n_clips_enc, d = w->tdims.n_state, V = w->tdims.n_vocab;
    for (int i = 0; i < n; i++) {
        const int T = token_offsets[i + 1] - token_offsets[i];
        const int sb = sample_begin_of ? sample_begin_of[i] : sample_begin_all;
        if (sb < 1 || T < sb || T > w->tdims.n_text_ctx) return pce_fail(c, PCE_E_INVALID, "clip %d: %d tokens (need %d..%d)", i, T, sb, w->tdims.n_text_ctx);
    }
    PCE_TRY(pad_token_rows(c, tokens, token_offsets, n, V, "token", 5, rows));
    std::vector<int> &tok = rows.tok, &tab = rows.tab;
    for (int i = 0; i < n; i++) tab[(size_t)4 * n + i] = sample_begin_of ? sample_begin_of[i] : sample_begin_all;
    PCE_HIP(c, w->g_last.reserve(sizeof(float) * (size_t)n * d));
    PCE_HIP(c, w->g_lastln.reserve(sizeof(op_t) * (size_t)(n + 128) * d + 4096));
    w->al_tab_host.clear();                                     // (d_tab / d_tokens are shared with pce_whisper_align_run: it uploads again)
    PCE_UPLOAD(c, w->d_tab, tab);
    PCE_UPLOAD(c, w->d_tokens, tok);
    if (vocab_mask) PCE_UPLOAD(c, w->g_mask, vocab_mask, (size_t)V, 64);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}
// Part 2, the launches: cross K / V of every layer (once per encoded batch), then one new position per sequence when the self-attention cache holds
// all but the last token of every prompt (`use_cache`), else the prefix pass, which fills that cache -> g_lastln [n][d] op_t.  The host's record
// of what the cache holds is brought up to date.
static int decode_prompts_to_lastln(pce_ctx *c, WhisperState *w, const int32_t *tokens, const int32_t *token_offsets, const TokenRows &rows, bool use_cache)
{
    const int n = w->n_clips_enc, d = w->tdims.n_state, L = w->tdims.n_layer, SPD = PREFIX_SP;
    const int T_pad = rows.T_pad;
    const std::vector<int> &t_len = rows.t_len;
    const int64_t Ma = (int64_t)n * W_CTX;
    const PrefixRun run = prefix_run(w, n, T_pad);
    const int *TL = run.TL;
    // ---- cross K / V of every layer, once per encoded batch
    const size_t xk_l = (size_t)Ma * d, xvt_l = (size_t)n * (size_t)d * AT_SP;
    if (w->g_xkv_clips != n) {
        PCE_HIP(c, w->g_xk.reserve(sizeof(op_t) * xk_l * (size_t)L + 4096));
        PCE_HIP(c, w->d_enc_bf16.reserve(sizeof(op_t) * (size_t)Ma * d + 4096));
        PCE_ZERO(op_t, c, w->g_xvt, xvt_l * (size_t)L, 2048);                                         // V^T columns 1500..AT_SP are read as zeros
        if (w->enc_bf16_clips != n)
            hipLaunchKernelGGL(k_f32_to_bf16, dim3((unsigned)div_up(Ma * d, 256)), dim3(256), 0, c->stream, w->final_out.as<float>(),
                               w->d_enc_bf16.as<op_t>(), Ma * d);
        for (int l = 0; l < L; l++) {
            const WhisperState::DLayer &ly = w->dlayers[(size_t)l];
            project_cross_kv(c, w->d_enc_bf16.as<op_t>(), (int)Ma, d, run.Wb + ly.xkv_w, run.Wf + ly.xkv_b, w->g_xk.as<op_t>() + xk_l * (size_t)l,
                             w->g_xvt.as<op_t>() + xvt_l * (size_t)l);
        }
        w->g_xkv_clips = n;
    }
    // ---- self-attention K / V cache [layer][clip][T_cap] (rows) / [layer][clip][d][512] (transposed)
    const int T_cap = w->tdims.n_text_ctx;
    const size_t sk_l = (size_t)n * T_cap * d, svt_l = (size_t)n * (size_t)d * SPD;
    if (w->g_cache_n != n || !w->g_sk.p) {
        PCE_ZERO(op_t, c, w->g_sk, sk_l * (size_t)L, 2048);
        PCE_ZERO(op_t, c, w->g_svt, svt_l * (size_t)L, 2048);
        PCE_ZERO(op_t, c, w->g_sv, sk_l * (size_t)L, 2048);
        w->g_cache_n = n; w->g_cache_len = -1; w->g_cache_tok.assign((size_t)n * T_cap, 0); w->g_cache_lens.assign((size_t)n, -1);
    }
    // incremental: every sequence extends what the cache holds for it by exactly one token (lengths may differ between sequences)
    bool incremental = w->g_cache_len >= 0 && use_cache;
    for (int i = 0; incremental && i < n; i++) {
        const int Li = t_len[(size_t)i];
        incremental = Li >= 2 && w->g_cache_lens[(size_t)i] == Li - 1 &&
                      memcmp(&w->g_cache_tok[(size_t)i * T_cap], &tokens[token_offsets[i]], sizeof(int) * (size_t)(Li - 1)) == 0;
    }
    if (incremental) {
        // ---- one new position per sequence: every GEMM has M = clips rows, the attention one query per (clip, head)
        std::vector<int> ct((size_t)8 * n);                     // new token | q_row0 | q_len | k_row0 | k_len | a_row0 | a_len | position
        for (int i = 0; i < n; i++) {
            const int pos_i = t_len[(size_t)i] - 1;
            ct[(size_t)i] = tokens[token_offsets[i] + pos_i]; ct[(size_t)n + i] = i; ct[(size_t)2 * n + i] = 1; ct[(size_t)3 * n + i] = i * T_cap;
            ct[(size_t)4 * n + i] = pos_i + 1; ct[(size_t)5 * n + i] = i * W_CTX; ct[(size_t)6 * n + i] = W_CTX; ct[(size_t)7 * n + i] = pos_i;
        }
        PCE_TRY(decode_incremental_reserve(c, w, n));
        PCE_PUT(c, w->g_c_tab.p, ct.data(), ct.size());
        PCE_HIP(c, hipStreamSynchronize(c->stream));
        decode_incremental_launches(c, w, n, w->g_c_tab.as<int>(), nullptr);
    } else {
    PCE_TRY(prefix_reserve_and_embed(c, w, run));
    for (int l = 0; l < L; l++) {
        const WhisperState::DLayer &ly = w->dlayers[(size_t)l];
        op_t *svt = w->g_svt.as<op_t>() + svt_l * (size_t)l;       // the prefix run fills the cache: V^T straight from the epilogue, K rows copied
        prefix_self_qkv(c, w, run, ly, svt);
        hipLaunchKernelGGL(k_cache_k, dim3((unsigned)div_up(run.Mt * d, 256)), dim3(256), 0, c->stream, w->d_qk.as<op_t>(), T_pad, TL, d, T_cap, n,
                           w->g_sk.as<op_t>() + sk_l * (size_t)l);
        hipLaunchKernelGGL(k_cache_v_rows, dim3((unsigned)(d / 32), (unsigned)div_up(T_pad, 32), (unsigned)n), dim3(256), 0, c->stream, svt, TL, d, T_cap, SPD, n,
                           w->g_sv.as<op_t>() + sk_l * (size_t)l);
        prefix_self_attention(c, w, run, ly, svt);
        prefix_cross_attention(c, w, run, w->g_xk.as<op_t>() + xk_l * (size_t)l, w->g_xvt.as<op_t>() + xvt_l * (size_t)l);
        prefix_cross_out_mlp(c, w, run, ly, false);               // (tiled fc1: the prefill has never been measured on the persistent kernel)
    }
    // ---- last position -> ln
    hipLaunchKernelGGL(k_gather_last, dim3((unsigned)div_up((int64_t)n * d, 256)), dim3(256), 0, c->stream, w->d_resid.as<float>(), TL, T_pad, d, n,
                       w->g_last.as<float>());
    launch_layernorm<op_t>(c, w->g_last.as<float>(), run.Wf + w->dln_w, run.Wf + w->dln_b, (int64_t)n, d, w->g_lastln.as<op_t>());
    }
    // the cache now holds every position of these prefixes
    for (int i = 0; i < n; i++) {
        memcpy(&w->g_cache_tok[(size_t)i * T_cap], &tokens[token_offsets[i]], sizeof(int) * (size_t)t_len[(size_t)i]);
        w->g_cache_lens[(size_t)i] = t_len[(size_t)i];
    }
    w->g_cache_len = 0;
    return PCE_OK;
}

// ---- From a step's logits to its tokens: the two launches decode_step_device, pce_whisper_decode_loop and pce_selftest_decode_rules (their test hook,
// pce_whisper_selftest.inc) make.  launch_decode_rules: one workgroup per sequence over logits [n][R.ld]; `tokens` holds one row of `pitch` ids per sequence
// (T_pad of a step's padded prompts, T_cap of the loop's table).  launch_step_advance: ONE workgroup carries the choices into the loop's tables.
// the loop's device-resident state: table [n][T_cap], len / ended [n], out_tok / out_lp [n][max_new], the step counter, n_ended [max_new]
struct DecodeLoopState { int *tok_table, *len, *ended, *out_tok; float *out_lp; int *ctr, *n_ended; };
static void launch_decode_rules(pce_ctx *c, int n, const float *logits, const int *tokens, const int *t_len, int pitch, const unsigned char *vmask, const DecRules &R,
                                const int *sample_begin_of, int *next, float *next_logprob, float *probe_prob, const int *sample_key)
{
    hipLaunchKernelGGL(k_decode_rules, dim3((unsigned)n), dim3(DR_T), 0, c->stream, logits, tokens, t_len, pitch, vmask, R, sample_begin_of, next, next_logprob,
                       probe_prob, sample_key);
}
static void launch_step_advance(pce_ctx *c, const DecodeLoopState &s, int n, int T_cap, int eot, int max_new, const int *next, const float *next_lp, int *ct)
{
    hipLaunchKernelGGL(k_step_advance, dim3(1), dim3(256), 0, c->stream, n, T_cap, eot, max_new, s.tok_table, s.len, next, next_lp, ct, s.ended, s.out_tok, s.out_lp,
                       s.ctr, s.n_ended);
}

static int decode_step_device(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules,
                              const uint8_t *vocab_mask, const pce_whisper_decode_opts *opts, bool want_probe)
{
    float probe_dummy = 0.f;
    float *probe_prob = want_probe ? &probe_dummy : nullptr;      // (only its non-nullness is consulted below)
    const int32_t sample_begin = opts->sample_begin_all;
    WhisperState *w = ws_of(c);
    if (!w->dec_loaded) return pce_fail(c, PCE_E_STATE, "pce_whisper_decode_step before pce_whisper_decoder_load");
    if (w->n_clips_enc < 0) return pce_fail(c, PCE_E_STATE, "run pce_whisper_encode_run first");
    if (w->tdims.n_state != w->dims.n_state) return pce_fail(c, PCE_E_INVALID, "decoder and encoder widths differ");
    PCE_HIP(c, hipSetDevice(c->device));
    const int n = w->n_clips_enc, d = w->tdims.n_state, V = w->tdims.n_vocab;
    if (rules->eot < 0 || rules->eot >= V || rules->timestamp_begin <= rules->eot || rules->timestamp_begin > V || (!opts->sample_begin && sample_begin < 1))
        return pce_fail(c, PCE_E_INVALID, "decoding rules: need 0 <= eot < timestamp_begin <= n_vocab, sample_begin >= 1");
    if (!(opts->temperature >= 0.f) || opts->probe_token >= V) return pce_fail(c, PCE_E_INVALID, "decoding options: temperature >= 0, probe_token < n_vocab");
    if (n == 0) return PCE_OK;
    const int64_t Vp = div_up(V, 128) * 128;
    PCE_HIP(c, w->g_logits.reserve(sizeof(float) * (size_t)n * (size_t)Vp));
    PCE_HIP(c, w->g_next.reserve((sizeof(int) + 2 * sizeof(float)) * (size_t)n));
    TokenRows rows;
    PCE_TRY(decode_stage_prompts(c, w, tokens, token_offsets, opts->sample_begin, sample_begin, vocab_mask, rows));
    KernelTimer timer(c, PCE_K_WHISPER_DECODE);
    PCE_TRY(decode_prompts_to_lastln(c, w, tokens, token_offsets, rows, !(opts->flags & 1)));
    // ---- logits = hidden . E^T (fp32, zero-initialised accumulator), the filters and the choice
    const int *T0 = w->d_tab.as<int>(), *TL = T0 + n;
    launch_gemm<EPI_F32>(c, w->g_lastln.as<op_t>(), d, 0, w->g_emb_bf16.as<op_t>(), n, (int)Vp, d, nullptr, w->g_logits.as<float>(), Vp, 0, 1);
    DecRules R{rules->eot, rules->timestamp_begin, V, (int)Vp, sample_begin, rules->max_initial_timestamp_index, opts->temperature, opts->seed_lo,
               opts->seed_hi, probe_prob ? opts->probe_token : -1};
    launch_decode_rules(c, n, w->g_logits.as<float>(), w->d_tokens.as<int>(), TL, rows.T_pad, w->g_mask.as<unsigned char>(), R, T0 + 4 * n, w->g_next.as<int>(),
                        reinterpret_cast<float *>(w->g_next.as<int>() + n), reinterpret_cast<float *>(w->g_next.as<int>() + 2 * n),
                        w->g_keys_n == n ? w->g_keys.as<int>() : nullptr);
    PCE_HIP(c, hipGetLastError());
    return PCE_OK;
}

// ---------------------------------------------------------------------------
// Language detection (openai-whisper decoding.py detect_language): the decoder over the one token <|startoftranscript|> per clip, then k_lang_probs
// (pce_decode_rules.inc) on the n_lang language rows of the tied embedding -- no output projection over the vocabulary, no k_decode_rules.
// ---------------------------------------------------------------------------
int pce_whisper_detect_language(pce_ctx *c, int32_t sot, int32_t lang_begin, int32_t n_lang, int32_t *ids, float *probs)
{
    if (!c) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (!w->dec_loaded) return pce_fail(c, PCE_E_STATE, "pce_whisper_detect_language before pce_whisper_decoder_load");
    if (w->n_clips_enc < 0) return pce_fail(c, PCE_E_STATE, "run pce_whisper_encode_run first");
    if (w->tdims.n_state != w->dims.n_state) return pce_fail(c, PCE_E_INVALID, "decoder and encoder widths differ");
    const int n = w->n_clips_enc, d = w->tdims.n_state, V = w->tdims.n_vocab;
    if (n_lang < 1 || n_lang > LANG_MAX) return pce_fail(c, PCE_E_INVALID, "language detection over %d tokens (1..%d)", n_lang, LANG_MAX);
    if (lang_begin < 0 || lang_begin > V - n_lang) return pce_fail(c, PCE_E_INVALID, "language tokens %d..%d leave the vocabulary of %d", lang_begin, lang_begin + n_lang - 1, V);
    if (sot < 0 || sot >= V) return pce_fail(c, PCE_E_INVALID, "token %d out of the vocabulary", sot);
    PCE_HIP(c, hipSetDevice(c->device));
    if (n == 0) return PCE_OK;
    std::vector<int32_t> tokens((size_t)n, sot), offsets((size_t)n + 1);
    for (int i = 0; i <= n; i++) offsets[(size_t)i] = i;
    PCE_HIP(c, w->g_lang.reserve((sizeof(float) * (size_t)n_lang + sizeof(int)) * (size_t)n));
    TokenRows rows;
    PCE_TRY(decode_stage_prompts(c, w, tokens.data(), offsets.data(), nullptr, 1, nullptr, rows));
    float *d_probs = w->g_lang.as<float>();
    int *d_ids = reinterpret_cast<int *>(d_probs + (size_t)n * n_lang);
    {
        KernelTimer timer(c, PCE_K_WHISPER_DECODE);
        // (never the incremental form: a one-token prompt extends nothing)
        PCE_TRY(decode_prompts_to_lastln(c, w, tokens.data(), offsets.data(), rows, false));
        hipLaunchKernelGGL(k_lang_probs, dim3((unsigned)n), dim3(LANG_T), 0, c->stream, w->g_lastln.as<op_t>(), w->g_emb_bf16.as<op_t>(), d, (int)lang_begin,
                           (int)n_lang, d_probs, d_ids);
        PCE_HIP(c, hipGetLastError());
    }
    // The cache now holds position 0 of every clip for the token `sot`, which is what any later prompt starts with; all the same the host's record of it is
    // dropped, so that the next decoding call runs its prompts through the prefix pass exactly as it does after a fresh pce_whisper_encode_run
    // (the cross K / V of the batch stay: they are what that call would compute first)
    w->g_cache_len = -1;
    if (ids) PCE_FETCH(c, ids, d_ids, (size_t)n);
    if (probs) PCE_FETCH(c, probs, d_probs, (size_t)n * n_lang);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

// ---------------------------------------------------------------------------
// Free-running decoding with the loop on the device (round 3).  pce_whisper_decode_step_ex round-trips every step through the
// host (tokens up, next token down, a synchronisation each way); here the prompts go up once, every later step reads what it
// needs -- the token it embeds, its position, the self-attention key count, which sequences have ended -- from tables the previous
// step's k_step_advance left on the device, and the host only looks at an "ended" counter every `check_every` steps.
// Same kernels, same filters, same counter-based sampling keys (seed, clip, position): token for token what the host-driven loop
// of Aligners/decoding.py produces (tests/test_gpu_aligner.py).
// ---------------------------------------------------------------------------
int pce_whisper_decode_loop(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules,
                                       const uint8_t *vocab_mask, const pce_whisper_decode_opts *opts, int32_t max_new, int32_t check_every,
                                       int32_t *out_tokens, float *out_logprobs, int32_t *out_steps, float *probe_prob)
{
    if (!c || !tokens || !token_offsets || !rules || !vocab_mask || !opts || !out_tokens || !out_steps) return PCE_E_INVALID;
    if (max_new < 1) return pce_fail(c, PCE_E_INVALID, "decode loop: max_new must be >= 1");
    if (check_every < 1) check_every = 4;
    WhisperState *w = ws_of(c);
    if (!w->dec_loaded) return pce_fail(c, PCE_E_STATE, "pce_whisper_decode_loop before pce_whisper_decoder_load");
    if (w->n_clips_enc < 0) return pce_fail(c, PCE_E_STATE, "run pce_whisper_encode_run first");
    const int n = w->n_clips_enc, d = w->tdims.n_state, V = w->tdims.n_vocab, T_cap = w->tdims.n_text_ctx;
    *out_steps = 0;
    if (n == 0) return PCE_OK;
    // (a sequence that fills the text context stops there -- k_step_advance -- as openai-whisper's loop breaks when tokens.shape[-1] > n_ctx
    // (decoding.py, DecodingTask._main_loop); the others go on: nothing is refused for what max_new MIGHT reach)
    PCE_HIP(c, hipSetDevice(c->device));
    KernelTimer loop_timer(c, PCE_K_DECODE_LOOP);
    // ---- step 0: the prompts (prefix run, or one more position when the cache already holds them); next token stays in g_next
    PCE_TRY(decode_step_device(c, tokens, token_offsets, rules, vocab_mask, opts, probe_prob != nullptr && opts->probe_token >= 0));
    PCE_TRY(decode_incremental_reserve(c, w, n));
    const int64_t Vp = div_up(V, 128) * 128;
    // ---- device-resident loop state
    const size_t n_state_ints = (size_t)n * T_cap + 3 * (size_t)n + (size_t)n * max_new + 8 + (size_t)max_new;
    PCE_HIP(c, w->g_loop.reserve(sizeof(int) * n_state_ints + sizeof(float) * (size_t)n * max_new + 256));
    int *tok_table = w->g_loop.as<int>(), *len = tok_table + (size_t)n * T_cap, *ended = len + n, *sb = ended + n, *out_tok = sb + n,
        *ctr = out_tok + (size_t)n * max_new, *n_ended = ctr + 8;
    float *out_lp = reinterpret_cast<float *>(n_ended + max_new);
    std::vector<int> h_tab((size_t)n * T_cap, 0), h_len((size_t)n), h_sb((size_t)n), ct((size_t)8 * n, 0);
    for (int i = 0; i < n; i++) {
        const int T = token_offsets[i + 1] - token_offsets[i];
        memcpy(&h_tab[(size_t)i * T_cap], &tokens[token_offsets[i]], sizeof(int) * (size_t)T);
        h_len[(size_t)i] = T; h_sb[(size_t)i] = opts->sample_begin ? opts->sample_begin[i] : opts->sample_begin_all;
        ct[(size_t)n + i] = i; ct[(size_t)2 * n + i] = 1; ct[(size_t)3 * n + i] = i * T_cap; ct[(size_t)5 * n + i] = i * W_CTX; ct[(size_t)6 * n + i] = W_CTX;
    }
    PCE_HIP(c, hipMemsetAsync(ended, 0, sizeof(int) * (n_state_ints - (size_t)n * T_cap - (size_t)n) + sizeof(float) * (size_t)n * max_new, c->stream));
    PCE_PUT(c, tok_table, h_tab.data(), h_tab.size());
    PCE_PUT(c, len, h_len.data(), (size_t)n);
    PCE_PUT(c, sb, h_sb.data(), (size_t)n);
    PCE_PUT(c, w->g_c_tab.p, ct.data(), ct.size());
    PCE_HIP(c, hipStreamSynchronize(c->stream));                 // (the host vectors are done with; the ONE upload of the window)
    int *CT = w->g_c_tab.as<int>();
    const int *next = w->g_next.as<int>();
    const float *next_lp = reinterpret_cast<const float *>(w->g_next.as<int>() + n);
    const DecodeLoopState state{tok_table, len, ended, out_tok, out_lp, ctr, n_ended};
    auto advance = [&]() { launch_step_advance(c, state, n, T_cap, (int)rules->eot, (int)max_new, next, next_lp, CT); };
    auto all_ended = [&](int step, bool *yes) -> int {
        int cnt = 0;
        PCE_FETCH(c, &cnt, n_ended + step, 1);
        PCE_HIP(c, hipStreamSynchronize(c->stream));
        *yes = cnt >= n;
        return PCE_OK;
    };
    advance();
    int steps = 1;
    bool stop = false;
    DecRules R{rules->eot, rules->timestamp_begin, V, (int)Vp, opts->sample_begin_all, rules->max_initial_timestamp_index, opts->temperature, opts->seed_lo,
               opts->seed_hi, -1};
    if (max_new > 1) PCE_TRY(all_ended(0, &stop));
    while (!stop && steps < max_new) {
        decode_incremental_launches(c, w, n, CT, ended);
        launch_gemm<EPI_F32>(c, w->g_lastln.as<op_t>(), d, 0, w->g_emb_bf16.as<op_t>(), n, (int)Vp, d, nullptr, w->g_logits.as<float>(), Vp, 0, 1);
        launch_decode_rules(c, n, w->g_logits.as<float>(), tok_table, len, T_cap, w->g_mask.as<unsigned char>(), R, sb, w->g_next.as<int>(),
                            reinterpret_cast<float *>(w->g_next.as<int>() + n), nullptr, w->g_keys_n == n ? w->g_keys.as<int>() : nullptr);
        advance();
        steps++;
        if (steps % check_every == 0 && steps < max_new) PCE_TRY(all_ended(steps - 1, &stop));
    }
    PCE_HIP(c, hipGetLastError());
    // ---- the ONE download of the window
    std::vector<int> h_out((size_t)n * max_new);
    std::vector<float> h_lp((size_t)n * max_new);
    PCE_FETCH(c, h_out.data(), out_tok, h_out.size());
    PCE_FETCH(c, h_lp.data(), out_lp, h_lp.size());
    if (probe_prob && opts->probe_token >= 0)
        PCE_FETCH(c, probe_prob, w->g_next.as<int>() + 2 * n, (size_t)n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++)
        for (int sidx = 0; sidx < max_new; sidx++) {
            // steps that never ran read as "already ended": end-of-text with a zero log-probability, what further steps would have produced
            out_tokens[(size_t)i * max_new + sidx] = sidx < steps ? h_out[(size_t)i * max_new + sidx] : rules->eot;
            if (out_logprobs) out_logprobs[(size_t)i * max_new + sidx] = sidx < steps ? h_lp[(size_t)i * max_new + sidx] : 0.f;
        }
    *out_steps = steps;
    w->g_cache_len = -1;                                         // the host's copy of the cached prefixes is stale: the next host-driven step re-runs its prefixes
    return PCE_OK;
}

} // namespace PCE_BUILD_NS
