// pce_encoder.inc -- the tiled transformer encoder layer walk that Whisper's audio encoder, BERT (pce_bert.inc) and wav2vec2 (pce_w2v.inc) share, and
// the Whisper encoder's entry points.  Included by pce_whisper_impl.inc behind the launchers the walk runs on.
namespace {
// One run of encoder_walk: M rows of width d in n_items attention items (clips, sequences, windows) of rows_per_item rows each
struct EncoderRun {
    int M, d, H, I, n_items, rows_per_item, vt_sp;      // H heads, I = the MLP's inner width, vt_sp = key columns of an item's V^T image
    const int *row0, *len;                              // device tables [n_items]: an item's first row and its length, for queries and keys alike
    float eps; double attn_flops; bool time_ln;         // the work the attention's timer counts; each LayerNorm under a PCE_K_LAYERNORM timer of its own
    float *resid; op_t *ln, *qk, *vt, *attn, *hidden;   // the stream [M][d]; LayerNorm output [M][d], Q | K [M][2d], V^T, attention output [M][d], MLP hidden [M][I]
    const op_t *Wb; const float *Wf;                    // the model's weight buffers (EncoderLayerW's offsets count from these)
};
// One layer's tensors from the blob cursor, in openai-whisper's order (ln_first: ln1, attention, ln2, MLP) or transformers' (attention, ln1, MLP, ln2)
static EncoderLayerW pack_encoder_layer(WeightPack &pk, const float *&p, size_t d, size_t I, bool ln_first, bool key_bias)
{
    EncoderLayerW ly;
    const auto ln = [&](size_t &w, size_t &b) { w = pk.vec(p, d); b = pk.vec(p, d); };
    if (ln_first) ln(ly.ln1_w, ly.ln1_b);
    const WeightPack::Attn a = pk.self_attention(p, d, key_bias);
    ly.qkv_w = a.qkv_w; ly.qkv_b = a.qkv_b; ly.out_w = a.out_w; ly.out_b = a.out_b;
    if (ln_first) ln(ly.ln2_w, ly.ln2_b); else ln(ly.ln1_w, ly.ln1_b);
    ly.m1_w = pk.mat(p, I * d); ly.m1_b = pk.vec(p, I); ly.m2_w = pk.mat(p, d * I); ly.m2_b = pk.vec(p, d);
    if (!ln_first) ln(ly.ln2_w, ly.ln2_b);
    return ly;
}

// The GEMM rule of a walk, a compile-time parameter: run<EPI> takes launch_gemm's arguments and says whether the product was launched.
// The product's rule always launches; wav2vec2's (W2vGemm, pce_w2v.inc) refuses a shape its kernel does not compute.
struct ProductGemm {
    template <int EPI, class... A> static bool run(pce_ctx *c, A... a) { launch_gemm<EPI>(c, a...); return true; }
};

// The layers of one encoder on the tiled kernels, in place on r.resid.  Pre-LN: x += proj(MHA(LN1(x))); x += W2 gelu(W1 LN2(x)).  Post-LN: r.ln holds
// LN(x) on entry, x = LN1(x + proj(MHA(x))); x = LN2(x + W2 gelu(W1 x)), each LayerNorm written back into the stream and into r.ln.  The LayerNorm in
// front of a post-LN stack and the one behind a pre-LN stack are the caller's.  Returns whether every product was launched.
// probe(layer, stage) is called behind every launch, in launch order (EncoderStage names the launch; its buffers: ES_LN_A r.ln; ES_QKV r.qk and r.vt;
// ES_ATTN r.attn; ES_X1 / ES_X2 r.resid; ES_LN_B / ES_LN_C r.ln, and r.resid where the form is post-LN; ES_HIDDEN r.hidden).  The product's probe is empty and
// compiles away; pce_selftest_encoder_walk's queues a copy of what the launch wrote.
enum EncoderStage { ES_LN_A, ES_QKV, ES_ATTN, ES_X1, ES_LN_B, ES_HIDDEN, ES_X2, ES_LN_C };
struct NoProbe { void operator()(int, EncoderStage) const {} };
template <class Gemm, class Probe = NoProbe>
static bool encoder_walk(pce_ctx *c, const EncoderRun &r, const std::vector<EncoderLayerW> &layers, bool pre_ln, Probe probe = Probe{})
{
    const int M = r.M, d = r.d, I = r.I;
    auto ln = [&](size_t w_off, size_t b_off) {
        std::optional<KernelTimer> kt;
        if (r.time_ln) kt.emplace(c, PCE_K_LAYERNORM);
        launch_layernorm<op_t>(c, r.resid, r.Wf + w_off, r.Wf + b_off, M, d, r.ln, r.eps, pre_ln ? nullptr : r.resid);
    };
    bool fit = true;
    int l = 0;
    for (const EncoderLayerW &ly : layers) {
        if (pre_ln) { ln(ly.ln1_w, ly.ln1_b); probe(l, ES_LN_A); }
        // Q | K go to the row-major [M][2d] buffer, V is written transposed per head: one launch sweeps the LayerNorm output once
        fit &= Gemm::template run<EPI_QKV>(c, r.ln, d, 0, r.Wb + ly.qkv_w, M, 3 * d, d, r.Wf + ly.qkv_b, r.qk, 2 * d, 0, 1,
                                           reinterpret_cast<const float *>(r.vt), r.rows_per_item, 2 * d, r.vt_sp);
        probe(l, ES_QKV);
        launch_attention_rows(c, r.n_items, r.H, r.rows_per_item, r.qk, 2 * d, r.qk + d, 2 * d, r.vt, r.vt_sp, r.row0, r.len, r.row0, r.len, r.attn, 0,
                              r.attn_flops);                     // keys beyond an item's length are masked (right padding)
        probe(l, ES_ATTN);
        fit &= Gemm::template run<EPI_RESID_F32>(c, r.attn, d, 0, r.Wb + ly.out_w, M, d, d, r.Wf + ly.out_b, r.resid, d, 0, 1);
        probe(l, ES_X1);
        if (pre_ln) ln(ly.ln2_w, ly.ln2_b); else ln(ly.ln1_w, ly.ln1_b);
        probe(l, ES_LN_B);
        fit &= Gemm::template run<EPI_GELU_BF16>(c, r.ln, d, 0, r.Wb + ly.m1_w, M, I, d, r.Wf + ly.m1_b, r.hidden, I, 0, 1);
        probe(l, ES_HIDDEN);
        fit &= Gemm::template run<EPI_RESID_F32>(c, r.hidden, I, 0, r.Wb + ly.m2_w, M, d, I, r.Wf + ly.m2_b, r.resid, d, 0, 1);
        probe(l, ES_X2);
        if (!pre_ln) { ln(ly.ln2_w, ly.ln2_b); probe(l, ES_LN_C); }
        l++;
    }
    return fit;
}
} // namespace

namespace PCE_BUILD_NS {

int pce_whisper_load(pce_ctx *c, const pce_whisper_dims *dims, const float *weights, int64_t n_floats)
{
    if (!c || !dims || !weights) return PCE_E_INVALID;
    const int d = dims->n_state, L = dims->n_layer, nm = dims->n_mels;
    if (d <= 0 || d % 128 || dims->n_head * 64 != d || L <= 0 || dims->n_ctx != W_CTX || nm <= 0 || nm > 128 || (nm % 8))
        return pce_fail(c, PCE_E_LIMIT, "unsupported encoder dims (need n_state %% 128 == 0, head size 64, n_ctx 1500, n_mels %% 8 == 0)");
    if (d > LN_D_MAX) return pce_fail(c, PCE_E_LIMIT, "encoder with n_state %d: the LayerNorm kernels hold at most %d", d, LN_D_MAX);
    // pce_whisper_encode_run takes the persistent GEMM for every projection when n_state % 256 == 0; its fc1 (N = 4 n_state) must fit it too
    if (c->sw.gemm_flat && d % F_T == 0 && 4 * d > F_N_MAX)
        return pce_fail(c, PCE_E_LIMIT, "encoder with n_state %d: the persistent GEMM's fc1 holds 4 n_state <= %d (PCE_GEMM_FLAT=0 at pce_create runs it on the "
                                        "tiled kernels)", d, F_N_MAX);
    const int64_t per_layer = 2LL * d + 4LL * d * d + 3LL * d + 2LL * d + 8LL * d * d + 5LL * d;
    const int64_t expect = (int64_t)d * nm * 3 + d + 3LL * d * d + d + L * per_layer + 2LL * d;
    if (n_floats != expect) return pce_fail(c, PCE_E_INVALID, "weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)expect);
    PCE_HIP(c, hipSetDevice(c->device));
    WhisperState *w = ws_of(c);
    PCE_TRY(lds_optins(c, w));
    w->dims = *dims; w->loaded = false; w->layers.assign((size_t)L, {});
    WeightPack pk;
    const float *p = weights;
    const size_t dd = (size_t)d * d;
    {   // conv1 [d][nm][3] -> [d][K1p] with k-major columns (k*nm + ci), zero padded to a multiple of 64
        const int K1 = 3 * nm, K1p = (int)div_up(K1, 64) * 64;
        w->c1_w = pk.mats.size(); pk.mats.resize(pk.mats.size() + (size_t)d * K1p, 0.f);
        for (int co = 0; co < d; co++)
            for (int ci = 0; ci < nm; ci++)
                for (int k = 0; k < 3; k++) pk.mats[w->c1_w + (size_t)co * K1p + (size_t)k * nm + ci] = p[((size_t)co * nm + ci) * 3 + k];
        p += (size_t)d * nm * 3;
        w->c1_b = pk.vec(p, (size_t)d);
    }
    {   // conv2 [d][d][3] -> [d][3 d]
        w->c2_w = pk.mats.size(); pk.mats.resize(pk.mats.size() + 3 * dd, 0.f);
        for (int co = 0; co < d; co++)
            for (int ci = 0; ci < d; ci++)
                for (int k = 0; k < 3; k++) pk.mats[w->c2_w + (size_t)co * 3 * d + (size_t)k * d + ci] = p[((size_t)co * d + ci) * 3 + k];
        p += 3 * dd;
        w->c2_b = pk.vec(p, (size_t)d);
    }
    for (EncoderLayerW &ly : w->layers) ly = pack_encoder_layer(pk, p, (size_t)d, (size_t)4 * d, true, false);
    w->lnp_w = pk.vec(p, (size_t)d); w->lnp_b = pk.vec(p, (size_t)d);
    // sinusoid positions [1500][d]
    std::vector<float> pos((size_t)W_CTX * d);
    {
        const int half = d / 2;
        const double inc = std::log(10000.0) / (half - 1);
        for (int t = 0; t < W_CTX; t++)
            for (int i = 0; i < half; i++) {
                const float inv = (float)std::exp(-inc * i);
                const float a = (float)t * inv;
                pos[(size_t)t * d + i] = std::sin(a); pos[(size_t)t * d + half + i] = std::cos(a);
            }
    }
    DevBuf tmp;
    PCE_TRY(upload_weights(c, pk, tmp, w->w_bf16, w->w_f32));
    PCE_UPLOAD(c, w->pos, pos);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    w->loaded = true;
    return PCE_OK;
}

int pce_whisper_encode_run(pce_ctx *c)
{
    if (!c) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (!w->loaded) return pce_fail(c, PCE_E_STATE, "pce_whisper_encode_run before pce_whisper_load");
    if (w->n_clips_mel < 0 || w->mel_nmels != w->dims.n_mels) return pce_fail(c, PCE_E_STATE, "run pce_logmel_run(n_mels of the model) first");
    PCE_HIP(c, hipSetDevice(c->device));
    const int d = w->dims.n_state, L = w->dims.n_layer, nm = w->dims.n_mels, H = w->dims.n_head;
    const int n = w->n_clips_mel;
    const int64_t M = (int64_t)n * W_CTX;
    if (M > INT32_MAX) return pce_fail(c, PCE_E_LIMIT, "too many clips for one encoder batch");
    const int K1p = (int)div_up(3 * nm, 64) * 64;
    const size_t c1_elems = (size_t)n * (W_FRAMES + 2) * (size_t)d + 4096;
    PCE_HIP(c, w->c1_out.reserve(sizeof(op_t) * c1_elems));
    PCE_HIP(c, w->resid.reserve(sizeof(float) * (size_t)M * d));
    PCE_HIP(c, w->ln_out.reserve(sizeof(op_t) * (size_t)M * d));
    PCE_HIP(c, w->qkv.reserve(sizeof(op_t) * (size_t)M * 2 * d));            // q | k, row-major
    const size_t vt_elems = (size_t)n * (size_t)d * AT_SP + 64;          // V^T [clip][head][64][AT_SP], pad keys stay zero
    {
        const size_t before = w->vt.cap;
        PCE_HIP(c, w->vt.reserve(sizeof(op_t) * vt_elems));
        if (w->vt.cap != before || w->vt_elems_zeroed < vt_elems) {
            PCE_HIP(c, hipMemsetAsync(w->vt.p, 0, sizeof(op_t) * vt_elems, c->stream));
            w->vt_elems_zeroed = vt_elems;
        }
    }
    PCE_HIP(c, w->attn.reserve(sizeof(op_t) * (size_t)M * d));
    PCE_HIP(c, w->hidden.reserve(sizeof(op_t) * (size_t)M * 4 * d));
    PCE_HIP(c, w->final_out.reserve(sizeof(float) * (size_t)M * d));
    const op_t *Wb = w->w_bf16.as<op_t>();
    const float *Wf = w->w_f32.as<float>();
    if (w->enc_tab_clips != n) {   // per-clip row tables of the attention descriptor: clip c owns rows [1500 c, 1500 c + 1500); they only depend on the
                                   // batch size, so a steady stream of equal batches uploads (and waits for) them once
        std::vector<int> tab((size_t)2 * n);
        for (int i = 0; i < n; i++) { tab[(size_t)i] = i * W_CTX; tab[(size_t)n + i] = W_CTX; }
        PCE_UPLOAD(c, w->enc_tab, tab);
        PCE_HIP(c, hipStreamSynchronize(c->stream));
        w->enc_tab_clips = n;
    }
    KernelTimer t(c, PCE_K_WHISPER_ENC);
    if (w->c1_out.cap != w->c1_zero_cap || w->c1_zero_d != d) {
        PCE_HIP(c, hipMemsetAsync(w->c1_out.p, 0, w->c1_out.cap, c->stream));
        w->c1_zero_cap = w->c1_out.cap; w->c1_zero_d = d;
    }
    // The stem leaves out the row tiles of the zero padding behind each clip's audio (ST_TILE; PCE_STEM_SKIP=0 at pce_create: two full launches), when both
    // convolutions run on the 128 x 128 kernel, whose tiles the ranges count.  INVARIANT: a c1_out row conv1 skipped is never read -- conv2 computes its tiles
    // [0, s) and its last one, which read conv1 tiles [0, 2 s) and [ST_C1_KEEP, 24), exactly what conv1 computed.  c1_out is reused across calls, so such a
    // row holds whatever an older batch left there.
    const bool stem_skip = c->sw.stem_skip && w->stem_tiles_c2 > 0 && gemm_choose<EPI_GELU_BF16>(c, GemmShape{W_FRAMES, d, K1p, nm, n, 0}) == GK_128 &&
                           gemm_choose<EPI_GELU_POS_F32>(c, GemmShape{W_CTX, d, 3 * d, 2 * (int64_t)d, n, 0}) == GK_128;
    GemmSkip skip1{nullptr, nullptr, 0, 0}, skip2 = skip1;       // a batch in which no clip leaves a tile out (full 30 s windows) runs the two full launches
    if (stem_skip) {
        PCE_HIP(c, w->stem_rep.reserve(sizeof(float) * (size_t)n * d));
        const int2 *sk = w->stem_skip.as<int2>();
        skip1 = GemmSkip{sk, nullptr, 0, w->stem_tiles_c1 * ST_TILE};
        skip2 = GemmSkip{sk + n, w->stem_rep.as<float>(), ST_TILE * ST_C2_LAST, w->stem_tiles_c2 * ST_TILE};
    }
    // conv1: per clip, A row t starts at padded row t (= t-1 unpadded), K = 3 n_mels (padded to K1p with zero weights)
    launch_gemm<EPI_GELU_BF16>(c, w->mel_tm.as<op_t>(), nm, (int64_t)(W_FRAMES + 2) * nm, Wb + w->c1_w, W_FRAMES, d, K1p, Wf + w->c1_b,
                               w->c1_out.as<op_t>() + d, d, (int64_t)(W_FRAMES + 2) * d, n, nullptr, 1, 0, AT_SP, stem_skip ? &skip1 : nullptr);
    // conv2 (stride 2): A row t' starts at padded row 2 t', K = 3 d, lda = 2 d; epilogue adds the positional embedding
    launch_gemm<EPI_GELU_POS_F32>(c, w->c1_out.as<op_t>(), 2 * (int64_t)d, (int64_t)(W_FRAMES + 2) * d, Wb + w->c2_w, W_CTX, d, 3 * d,
                                  Wf + w->c2_b, w->resid.as<float>(), d, (int64_t)W_CTX * d, n, w->pos.as<float>(), W_CTX, 0, AT_SP, stem_skip ? &skip2 : nullptr);
    if (stem_skip)         // the skipped conv2 rows: the repeated row's accumulators through conv2's own epilogue expression, plus each row's positions
                           // (no timer id of its own: it runs inside the whisper_encoder bracket; d % 128 == 0 by pce_whisper_load, pos is [W_CTX][d])
        hipLaunchKernelGGL(k_stem_fill, dim3((unsigned)(ST_TILE * ST_C2_LAST / SF_ROWS), (unsigned)n), dim3(256), 0, c->stream, skip2.tiles, w->stem_rep.as<float>(),
                           Wf + w->c2_b, w->pos.as<float>(), d, w->resid.as<float>());
    // The big projections run on the persistent 256 x 256 kernel when the MODEL's shape allows it (n_state % 256 == 0; any batch size,
    // one clip included: the arithmetic of a clip does not depend on what it is batched with).  On that path a branch (attention projection, MLP) leaves its output as a op_t row block and the residual add is fused
    // into the LayerNorm that follows (k_add_layernorm): one pass over the residual stream instead of the GEMM's read-modify-write
    // plus the LayerNorm's read.
    const bool flat = c->sw.gemm_flat && d % F_T == 0 && gemm_flat_offsets_fit(M, 4 * d, 4 * d, 4 * d, 0, 0) &&
                      gemm_flat_offsets_fit(M, d, d, 0, W_CTX, AT_SP);
    if (flat) PCE_HIP(c, w->d_enc_bf16.reserve(sizeof(op_t) * (size_t)M * d + 4096));
    // mid = the pass after the attention projection (x = resid + delta feeds ln2, the stream is not written), else the pass at the end of
    // the layer (x = (resid + delta) + delta2 is written back and feeds the next layer's ln1, or ln_post -> the fp32 encoder output)
    // resid16: the 16-bit residual stream of the flat path (fp16 operands only; pce_whisper_set_operands(PCE_OPERANDS_F16_RESID16)): layer 0 reads
    // the fp32 stem output and leaves the stream in w->resid16, the later layers read and write that
    const bool resid16 = flat && c->resid16 && PCE_OP_INDEX == 1;
    if (resid16) PCE_HIP(c, w->resid16.reserve(sizeof(op_t) * (size_t)M * d));
    // fused (resid16 unless PCE_RESID_EPILOGUE=0 at pce_create): the attention projection and fc2 add their rounded output to the 16-bit stream in
    // their epilogue (FEPI_RESID, in place in w->resid16: x1 = r16(x + r16(acc + bias)), x2 likewise -- the roundings k_add_layernorm makes), the
    // two passes of a layer are LayerNorm only (one read of the stream, one write of ln_out) and no branch output is stored; layer 0's
    // k_layernorm, which reads the fp32 stem output and rounds it on the way in, leaves that rounded copy in w->resid16
    // (PCE_RESID_EPILOGUE=2, the per-shape A/B: only fc2 is fused; the attention projection stores its output and the pass after it adds it and writes
    //  x1 back into the stream, which fc2's epilogue then reads)
    const bool fused = resid16 && c->sw.resid_epilogue != 0, fused_out = fused && c->sw.resid_epilogue == 1;
    if (flat && !fused_out) PCE_HIP(c, w->delta.reserve(sizeof(op_t) * (size_t)M * d));
    if (flat && !fused) PCE_HIP(c, w->delta2.reserve(sizeof(op_t) * (size_t)M * d));
    auto add_ln = [&](size_t w_off, size_t b_off, bool mid, bool last, bool first_layer) {
        KernelTimer kt(c, PCE_K_ADD_LAYERNORM);
        const op_t *d2 = mid ? nullptr : w->delta2.as<op_t>();
        float *r32 = w->resid.as<float>(); op_t *r16 = w->resid16.as<op_t>();
        const float *lw = Wf + w_off, *lb = Wf + b_off;
        const int wr = mid ? 0 : 1;
        if (fused && mid && !fused_out) {
            launch_add_layernorm<op_t, op_t, op_t>(c, r16, r16, w->delta.as<op_t>(), nullptr, 1, lw, lb, M, d, w->ln_out.as<op_t>(), 1e-5f, nullptr);
            return;
        }
        if (fused) {     // LayerNorm of the stream as the epilogues left it
            if (last) launch_add_layernorm0<float>(c, r16, lw, lb, M, d, w->final_out.as<float>(), 1e-5f, w->d_enc_bf16.as<op_t>());
            else launch_add_layernorm0<op_t>(c, r16, lw, lb, M, d, w->ln_out.as<op_t>(), 1e-5f, nullptr);
            return;
        }
        if (last) {      // ln_post: the fp32 encoder output + the op_t copy the decoder's cross K / V projections read
            float *fo = w->final_out.as<float>(); op_t *eo = w->d_enc_bf16.as<op_t>();
            if (!resid16) launch_add_layernorm<float, float, float>(c, r32, r32, w->delta.as<op_t>(), d2, 1, lw, lb, M, d, fo, 1e-5f, eo);
            else if (first_layer) launch_add_layernorm<float, float, op_t>(c, r32, r16, w->delta.as<op_t>(), d2, 1, lw, lb, M, d, fo, 1e-5f, eo);
            else launch_add_layernorm<float, op_t, op_t>(c, r16, r16, w->delta.as<op_t>(), d2, 1, lw, lb, M, d, fo, 1e-5f, eo);
        } else {
            op_t *lo = w->ln_out.as<op_t>();
            if (!resid16) launch_add_layernorm<op_t, float, float>(c, r32, r32, w->delta.as<op_t>(), d2, wr, lw, lb, M, d, lo, 1e-5f, nullptr);
            else if (first_layer) launch_add_layernorm<op_t, float, op_t>(c, r32, r16, w->delta.as<op_t>(), d2, wr, lw, lb, M, d, lo, 1e-5f, nullptr);
            else launch_add_layernorm<op_t, op_t, op_t>(c, r16, r16, w->delta.as<op_t>(), d2, wr, lw, lb, M, d, lo, 1e-5f, nullptr);
        }
    };
    const int *row0 = w->enc_tab.as<int>(), *len = row0 + n;
    const double attn_flops = 4.0 * W_CTX * (double)W_CTX * d * n;
    if (flat) {            // the persistent GEMM: a projection that does not fit it is an error
        for (int l = 0; l < L; l++) {
            const EncoderLayerW &ly = w->layers[(size_t)l];
            if (l == 0) {
                KernelTimer kt(c, PCE_K_LAYERNORM);
                launch_layernorm<op_t>(c, w->resid.as<float>(), Wf + ly.ln1_w, Wf + ly.ln1_b, M, d, w->ln_out.as<op_t>(), 1e-5f, nullptr, resid16 ? 1 : 0,
                                       fused ? w->resid16.as<op_t>() : nullptr);
            }
            // Q | K go to the row-major [M][2d] buffer, V is written transposed per head: one launch sweeps the LayerNorm output once
            if (!launch_gemm_flat<FEPI_SPLIT>(c, w->ln_out.as<op_t>(), Wb + ly.qkv_w, Wf + ly.qkv_b, w->qkv.as<op_t>(), (int)M, 3 * d, d, 2 * d, W_CTX, AT_SP,
                                              PCE_K_GEMM_FLAT_QKV, w->vt.as<op_t>(), 2 * d))
                return pce_fail(c, PCE_E_LIMIT, "Q | K | V projection does not fit the 256 x 256 kernel");
            launch_attention_rows(c, n, H, W_CTX, w->qkv.as<op_t>(), 2 * d, w->qkv.as<op_t>() + d, 2 * d, w->vt.as<op_t>(), AT_SP, row0, len, row0, len,
                                  w->attn.as<op_t>(), 0, attn_flops);
            op_t *const r16 = w->resid16.as<op_t>();
            if (!(fused_out ? launch_gemm_flat<FEPI_RESID>(c, w->attn.as<op_t>(), Wb + ly.out_w, Wf + ly.out_b, r16, (int)M, d, d, d, 1, 0, PCE_K_GEMM_FLAT_OUT, nullptr, 0, r16)
                            : launch_gemm_flat<FEPI_BF16>(c, w->attn.as<op_t>(), Wb + ly.out_w, Wf + ly.out_b, w->delta.as<op_t>(), (int)M, d, d, d, 1, 0, PCE_K_GEMM_FLAT_OUT)))
                return pce_fail(c, PCE_E_LIMIT, "attention projection does not fit the 256 x 256 kernel");
            add_ln(ly.ln2_w, ly.ln2_b, true, false, l == 0);
            if (!launch_gemm_flat<FEPI_GELU>(c, w->ln_out.as<op_t>(), Wb + ly.m1_w, Wf + ly.m1_b, w->hidden.as<op_t>(), (int)M, 4 * d, d, 4 * d, 1, 0, PCE_K_GEMM_FLAT_FC1) ||
                !(fused ? launch_gemm_flat<FEPI_RESID>(c, w->hidden.as<op_t>(), Wb + ly.m2_w, Wf + ly.m2_b, r16, (int)M, d, 4 * d, d, 1, 0, PCE_K_GEMM_FLAT_FC2, nullptr, 0, r16)
                        : launch_gemm_flat<FEPI_BF16>(c, w->hidden.as<op_t>(), Wb + ly.m2_w, Wf + ly.m2_b, w->delta2.as<op_t>(), (int)M, d, 4 * d, d, 1, 0, PCE_K_GEMM_FLAT_FC2)))
                return pce_fail(c, PCE_E_LIMIT, "MLP does not fit the 256 x 256 kernel");
            if (l + 1 < L) add_ln(w->layers[(size_t)l + 1].ln1_w, w->layers[(size_t)l + 1].ln1_b, false, false, l == 0);
            else add_ln(w->lnp_w, w->lnp_b, false, true, l == 0);
        }
    } else {               // the tiled kernels: the shared walk (pre-LN), then ln_post into the fp32 encoder output
        const EncoderRun r{(int)M, d, H, 4 * d, n, W_CTX, AT_SP, row0, len, 1e-5f, attn_flops, true, w->resid.as<float>(), w->ln_out.as<op_t>(),
                           w->qkv.as<op_t>(), w->vt.as<op_t>(), w->attn.as<op_t>(), w->hidden.as<op_t>(), Wb, Wf};
        encoder_walk<ProductGemm>(c, r, w->layers, true);
        KernelTimer kt(c, PCE_K_LAYERNORM);
        launch_layernorm<float>(c, w->resid.as<float>(), Wf + w->lnp_w, Wf + w->lnp_b, M, d, w->final_out.as<float>());
    }
    PCE_HIP(c, hipGetLastError());
    w->n_clips_enc = n; w->g_xkv_clips = -1; w->g_cache_len = -1; w->g_keys_n = 0; w->enc_bf16_clips = flat ? n : -1;
    return PCE_OK;
}

int pce_whisper_encode_fetch(pce_ctx *c, int32_t clip, float *out)
{
    if (!c || !out) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (w->n_clips_enc < 0) return pce_fail(c, PCE_E_STATE, "pce_whisper_encode_fetch before pce_whisper_encode_run");
    if (clip < 0 || clip >= w->n_clips_enc) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    const size_t per = (size_t)W_CTX * (size_t)w->dims.n_state;
    PCE_FETCH(c, out, w->final_out.as<float>() + per * (size_t)clip, per);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

} // namespace PCE_BUILD_NS
