// pce_bert.inc -- the break-prediction token classifier (included by pce_whisper_impl.inc after pce_whisper_decoder.inc: it runs on that file's
// GEMM / attention / LayerNorm launchers and pads its token rows as the decoder does, pad_token_rows).
namespace {
// BERT embeddings: word[id] + token_type[0] + position[t] (the LayerNorm follows as its own launch)
__global__ void k_bert_embed(const int *__restrict__ tokens /* [seqs][T_pad] */, const float *__restrict__ word, const float *__restrict__ pos,
                             const float *__restrict__ type0, int T_pad, int n_pos, int d, int64_t rows, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * d) return;
    const int64_t m = i / d; const int col = (int)(i - m * d);
    int t = (int)(m % T_pad); if (t >= n_pos) t = n_pos - 1;        // pad rows: any finite value
    out[i] = (word[(int64_t)tokens[m] * d + col] + type0[col]) + pos[(int64_t)t * d + col];
}
} // namespace

// ---------------------------------------------------------------------------
// Break-prediction token classifier: BertForTokenClassification forward (post-LN encoder layers on the same GEMM /
// attention / LayerNorm kernels as the Whisper encoder; Code/baseline_models/pause_bert.py:127-132).
// ---------------------------------------------------------------------------
namespace PCE_BUILD_NS {

int pce_bert_load(pce_ctx *c, const pce_bert_dims *dims, const float *weights, int64_t n_floats)
{
    if (!c || !dims || !weights) return PCE_E_INVALID;
    const int d = dims->n_state, L = dims->n_layer, V = dims->n_vocab, P = dims->n_pos, TY = dims->n_type, NL = dims->n_labels;
    if (d <= 0 || d % 128 || dims->n_head * 64 != d || L <= 0 || V <= 0 || P <= 0 || P > 512 || TY <= 0 || NL <= 0 || NL > 128)
        return pce_fail(c, PCE_E_LIMIT, "unsupported BERT dims (need n_state %% 128 == 0, head size 64, n_pos <= 512, n_labels <= 128)");
    if (d > LN_D_MAX) return pce_fail(c, PCE_E_LIMIT, "BERT with n_state %d: the LayerNorm kernels hold at most %d", d, LN_D_MAX);
    const int64_t dd = (int64_t)d * d;
    const int64_t per_layer = 4 * (dd + d) + 2LL * d + (4 * dd + 4LL * d) + (4 * dd + d) + 2LL * d;
    const int64_t expect = ((int64_t)V + P + TY) * d + 2LL * d + L * per_layer + (int64_t)NL * (d + 1);
    if (n_floats != expect) return pce_fail(c, PCE_E_INVALID, "BERT weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)expect);
    PCE_HIP(c, hipSetDevice(c->device));
    WhisperState::Bert &b = ws_of(c)->bert;
    b.dims = *dims; b.loaded = false; b.n_seq = -1; b.layers.assign((size_t)L, {});
    WeightPack pk;
    const float *p = weights;
    const float *word = p; p += (size_t)V * d;
    const float *pos = p; p += (size_t)P * d;
    const float *type = p; p += (size_t)TY * d;
    b.lne_w = pk.vec(p, (size_t)d); b.lne_b = pk.vec(p, (size_t)d);
    for (EncoderLayerW &ly : b.layers) ly = pack_encoder_layer(pk, p, (size_t)d, (size_t)4 * d, false, true);
    {   // classifier [n_labels][d] padded with zero rows to one 128-column GEMM tile
        std::vector<float> cw((size_t)128 * d, 0.f), cb(128, 0.f);
        memcpy(cw.data(), p, sizeof(float) * (size_t)NL * d); p += (size_t)NL * d;
        memcpy(cb.data(), p, sizeof(float) * (size_t)NL); p += NL;
        b.cls_w = pk.mat_at(cw.data(), cw.size()); b.cls_b = pk.vec_at(cb.data(), cb.size());
    }
    DevBuf tmp;
    PCE_TRY(upload_weights(c, pk, tmp, b.w_bf16, b.w_f32));
    PCE_UPLOAD(c, b.word, word, (size_t)V * d);
    PCE_UPLOAD(c, b.pos, pos, (size_t)P * d);
    PCE_UPLOAD(c, b.type0, type, (size_t)d);     // token_type_ids = 0
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    b.loaded = true;
    return PCE_OK;
}

int pce_bert_run(pce_ctx *c, const int32_t *input_ids, const int32_t *offsets, int32_t n_seq)
{
    if (!c || !input_ids || !offsets || n_seq < 0) return PCE_E_INVALID;
    WhisperState::Bert &b = ws_of(c)->bert;
    if (!b.loaded) return pce_fail(c, PCE_E_STATE, "pce_bert_run before pce_bert_load");
    PCE_HIP(c, hipSetDevice(c->device));
    const int d = b.dims.n_state, H = b.dims.n_head, V = b.dims.n_vocab, n = n_seq, SPD = 512;
    b.n_seq = -1;
    for (int i = 0; i < n; i++) {
        const int T = offsets[i + 1] - offsets[i];
        if (T < 1 || T > b.dims.n_pos) return pce_fail(c, PCE_E_INVALID, "sequence %d: %d tokens (need 1..%d)", i, T, b.dims.n_pos);
    }
    if (n == 0) { b.lens.clear(); b.n_seq = 0; return PCE_OK; }
    TokenRows rows;                                              // tables: [row0 | length]
    PCE_TRY(pad_token_rows(c, input_ids, offsets, n, V, "token id", 2, rows));
    b.lens = rows.t_len;
    const int T_pad = rows.T_pad; const int64_t M = (int64_t)n * T_pad;
    const std::vector<int> &tab = rows.tab, &tok = rows.tok;
    PCE_HIP(c, b.resid.reserve(sizeof(float) * (size_t)M * d));
    PCE_HIP(c, b.ln.reserve(sizeof(op_t) * (size_t)M * d + 4096));
    PCE_HIP(c, b.qk.reserve(sizeof(op_t) * (size_t)M * 2 * d + 4096));
    PCE_HIP(c, b.hidden.reserve(sizeof(op_t) * (size_t)M * 4 * d + 4096));
    PCE_HIP(c, b.logits.reserve(sizeof(float) * (size_t)M * 128));
    const size_t vt_elems = (size_t)n * (size_t)d * SPD + 64;
    PCE_UPLOAD(c, b.tab, tab);
    PCE_UPLOAD(c, b.tokens, tok);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    // the attention kernel writes the rows of real tokens only and V^T columns beyond T_pad are never written: no stale bits
    PCE_ZERO(op_t, c, b.attn, (size_t)M * d + 2048);
    PCE_ZERO(op_t, c, b.vt, vt_elems);
    const int *T0 = b.tab.as<int>(), *TL = T0 + n;
    const op_t *Wb = b.w_bf16.as<op_t>();
    const float *Wf = b.w_f32.as<float>();
    const float eps = 1e-12f;                                    // BertConfig.layer_norm_eps
    KernelTimer timer(c, PCE_K_BERT);
    hipLaunchKernelGGL(k_bert_embed, dim3((unsigned)div_up(M * d, 256)), dim3(256), 0, c->stream, b.tokens.as<int>(), b.word.as<float>(),
                       b.pos.as<float>(), b.type0.as<float>(), T_pad, b.dims.n_pos, d, M, b.resid.as<float>());
    // the embedding LayerNorm opens the post-LN stack: resid <- LN(resid) (fp32, in place) and its op_t copy
    launch_layernorm<op_t>(c, b.resid.as<float>(), Wf + b.lne_w, Wf + b.lne_b, M, d, b.ln.as<op_t>(), eps, b.resid.as<float>());
    const EncoderRun r{(int)M, d, H, 4 * d, n, T_pad, SPD, T0, TL, eps, 0.0, false, b.resid.as<float>(), b.ln.as<op_t>(), b.qk.as<op_t>(), b.vt.as<op_t>(),
                       b.attn.as<op_t>(), b.hidden.as<op_t>(), Wb, Wf};
    encoder_walk<ProductGemm>(c, r, b.layers, false);
    // classifier: logits[M][128] = 0 + hidden . W^T + b (the first n_labels columns are real)
    launch_gemm<EPI_F32>(c, b.ln.as<op_t>(), d, 0, Wb + b.cls_w, (int)M, 128, d, Wf + b.cls_b, b.logits.as<float>(), 128, 0, 1);
    PCE_HIP(c, hipGetLastError());
    b.n_seq = n; b.T_pad = T_pad;
    return PCE_OK;
}

int pce_bert_fetch(pce_ctx *c, int32_t seq, float *logits, int32_t *labels)
{
    if (!c) return PCE_E_INVALID;
    WhisperState::Bert &b = ws_of(c)->bert;
    if (b.n_seq < 0) return pce_fail(c, PCE_E_STATE, "pce_bert_fetch before pce_bert_run");
    if (seq < 0 || seq >= b.n_seq) return pce_fail(c, PCE_E_INVALID, "sequence out of range");
    PCE_HIP(c, hipSetDevice(c->device));
    const int T = b.lens[(size_t)seq], NL = b.dims.n_labels;
    std::vector<float> rows((size_t)T * 128);
    PCE_FETCH(c, rows.data(), b.logits.as<float>() + (size_t)seq * b.T_pad * 128, rows.size());
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    for (int t = 0; t < T; t++) {
        int best = 0;
        for (int k = 0; k < NL; k++) {
            const float v = rows[(size_t)t * 128 + k];
            if (logits) logits[(size_t)t * NL + k] = v;
            if (v > rows[(size_t)t * 128 + best]) best = k;          // first maximum, as argmax
        }
        if (labels) labels[t] = best;
    }
    return PCE_OK;
}

} // namespace PCE_BUILD_NS
