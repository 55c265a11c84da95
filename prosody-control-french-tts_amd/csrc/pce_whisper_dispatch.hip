// pce_whisper_dispatch.hip -- the Whisper / BERT / wav2vec2 entry points of include/pce.h: each forwards to the build of pce_whisper_impl.inc (and the .inc files it includes)
// (bf16 or fp16 operands) the context has selected.  The two builds keep separate state (weights, buffers): switching the operand
// type means loading the weights again.
#include "pce_internal.h"

#define PCE_BOTH(ret, name, params)  extern "C" { ret name##_bf16 params; ret name##_f16 params; }
#define PCE_FWD(name, ...) ((c && c->whisper_ops >= 1) ? name##_f16(__VA_ARGS__) : name##_bf16(__VA_ARGS__))

PCE_BOTH(int, pce_logmel_run, (pce_ctx *, int32_t))
PCE_BOTH(int, pce_logmel_run_at, (pce_ctx *, int32_t, const int64_t *))
PCE_BOTH(int, pce_logmel_fetch, (pce_ctx *, int32_t, float *))
PCE_BOTH(int, pce_selftest_logmel_image, (pce_ctx *, int32_t, uint16_t *))
PCE_BOTH(int, pce_whisper_load, (pce_ctx *, const pce_whisper_dims *, const float *, int64_t))
PCE_BOTH(int, pce_whisper_encode_run, (pce_ctx *))
PCE_BOTH(int, pce_whisper_encode_fetch, (pce_ctx *, int32_t, float *))
PCE_BOTH(int, pce_selftest_attention, (pce_ctx *, const uint16_t *, const uint16_t *, const uint16_t *, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, uint16_t *, int32_t *))
PCE_BOTH(int, pce_selftest_attention_ragged, (pce_ctx *, const uint16_t *, const uint16_t *, const uint16_t *, int32_t, int32_t, const int32_t *, const int32_t *, int32_t, int32_t, uint16_t *, int64_t, int32_t *))
PCE_BOTH(int, pce_selftest_attn1, (pce_ctx *, int32_t, int32_t, int32_t, const uint16_t *, int64_t, uint16_t *, int64_t, uint16_t *, int64_t, const int32_t *, const int32_t *, const int32_t *, int32_t, uint16_t *, int64_t))
PCE_BOTH(int, pce_selftest_align_matrix, (pce_ctx *, int32_t, int32_t, const uint16_t *, int64_t, const uint16_t *, int64_t, int32_t, const int32_t *, const int32_t *,
                                           const int32_t *, int32_t, int32_t, int32_t, int32_t, float, float *, int64_t, float *, int64_t, double *, int64_t))
PCE_BOTH(int, pce_selftest_decode_rules, (pce_ctx *, int32_t, int32_t, int32_t, int32_t, const float *, int64_t, const int32_t *, const int32_t *, int32_t, int32_t, const int32_t *,
                                           int32_t, const pce_whisper_decode_rules *, const uint8_t *, int64_t, float, uint32_t, uint32_t, int32_t, const int32_t *, int32_t,
                                           int32_t *, float *, float *, int64_t, int32_t *, int64_t, int32_t *, int64_t))
PCE_BOTH(int, pce_selftest_gemm, (pce_ctx *, const uint16_t *, const uint16_t *, const float *, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, uint16_t *))
PCE_BOTH(int, pce_selftest_gemm_resid, (pce_ctx *, const uint16_t *, const uint16_t *, const float *, uint16_t *, int32_t, int32_t, int32_t))
PCE_BOTH(int, pce_selftest_xattn, (pce_ctx *, const float *, const float *, const float *, const uint16_t *, const float *, const uint16_t *, const uint16_t *, const float *, const uint16_t *, const int32_t *, int32_t, int32_t, int32_t, int32_t, int32_t, uint16_t *))
PCE_BOTH(int, pce_selftest_gemm_tiled, (pce_ctx *, int32_t, int32_t, const uint16_t *, int64_t, int64_t, int64_t, int32_t, const uint16_t *, const float *, int32_t, int32_t,
                                         int32_t, void *, int64_t, int64_t, int64_t, const float *, int32_t, int32_t, int32_t, int32_t, uint16_t *, int64_t, int32_t *))
PCE_BOTH(int, pce_selftest_layernorm, (pce_ctx *, int32_t, int32_t, int32_t, const void *, const uint16_t *, const uint16_t *, const float *, const float *, float, int32_t,
                                        void *, void *, uint16_t *))
PCE_BOTH(int, pce_whisper_decoder_load, (pce_ctx *, const pce_whisper_text_dims *, const float *, int64_t))
PCE_BOTH(int, pce_whisper_align_run, (pce_ctx *, const int32_t *, const int32_t *, const int32_t *, int32_t, const uint8_t *, int32_t, float))
PCE_BOTH(int, pce_whisper_align_fetch, (pce_ctx *, int32_t, int32_t *, int32_t *, int32_t *, double *))
PCE_BOTH(int, pce_whisper_align_shape, (pce_ctx *, int32_t, int32_t *, int32_t *))
PCE_BOTH(int, pce_whisper_align_paths_enqueue, (pce_ctx *, int32_t, int32_t *, int32_t *))
PCE_BOTH(int, pce_whisper_align_paths_wait, (pce_ctx *, int32_t, int32_t *, int32_t *, int32_t *))
PCE_BOTH(int, pce_whisper_sample_keys, (pce_ctx *, const int32_t *, int32_t))
PCE_BOTH(int, pce_whisper_decode_step, (pce_ctx *, const int32_t *, const int32_t *, int32_t, const pce_whisper_decode_rules *, const uint8_t *, int32_t *, float *))
PCE_BOTH(int, pce_whisper_decode_step_ex, (pce_ctx *, const int32_t *, const int32_t *, const pce_whisper_decode_rules *, const uint8_t *, const pce_whisper_decode_opts *, int32_t *, float *, float *))
PCE_BOTH(int, pce_whisper_decode_loop, (pce_ctx *, const int32_t *, const int32_t *, const pce_whisper_decode_rules *, const uint8_t *, const pce_whisper_decode_opts *, int32_t, int32_t, int32_t *, float *, int32_t *, float *))
PCE_BOTH(int, pce_whisper_detect_language, (pce_ctx *, int32_t, int32_t, int32_t, int32_t *, float *))
PCE_BOTH(int, pce_bert_load, (pce_ctx *, const pce_bert_dims *, const float *, int64_t))
PCE_BOTH(int, pce_bert_run, (pce_ctx *, const int32_t *, const int32_t *, int32_t))
PCE_BOTH(int, pce_bert_fetch, (pce_ctx *, int32_t, float *, int32_t *))
PCE_BOTH(int, pce_w2v_check, (const pce_w2v_dims *, int64_t, char *, size_t))
PCE_BOTH(int, pce_w2v_load, (pce_ctx *, const pce_w2v_dims *, const float *, int64_t))
PCE_BOTH(int, pce_w2v_run, (pce_ctx *, const pce_w2v_plan *))
PCE_BOTH(int, pce_w2v_shape, (pce_ctx *, int32_t, int64_t *, int32_t *))
PCE_BOTH(int, pce_w2v_fetch, (pce_ctx *, int32_t, float *))
PCE_BOTH(int, pce_w2v_device, (pce_ctx *, const float **, const int64_t **, const int32_t **, int32_t *))
PCE_BOTH(int, pce_selftest_w2v_wave, (pce_ctx *, const int16_t *, int64_t, int32_t, int32_t, int32_t, int32_t, int32_t, const float *, const float *, const float *, const float *, uint16_t *))
PCE_BOTH(int, pce_selftest_w2v_lngelu, (pce_ctx *, const uint16_t *, int32_t, int32_t, const float *, const float *, float, int32_t, uint16_t *))
PCE_BOTH(int, pce_selftest_w2v_posconv, (pce_ctx *, const float *, int32_t, int32_t, int32_t, int32_t, const uint16_t *, const float *, float *))
void pce_whisper_free_bf16(pce_ctx *c);
void pce_whisper_free_f16(pce_ctx *c);

void pce_whisper_free(pce_ctx *c) { pce_whisper_free_bf16(c); pce_whisper_free_f16(c); }

extern "C" {

int pce_whisper_set_operands(pce_ctx *c, int32_t operand_type)
{
    if (!c) return PCE_E_INVALID;
    if (operand_type != PCE_OPERANDS_BF16 && operand_type != PCE_OPERANDS_FP16 && operand_type != PCE_OPERANDS_F16_RESID16)
        return pce_fail(c, PCE_E_INVALID, "operand type %d (0 = bf16, 1 = fp16, 2 = fp16 with the fp16 residual stream)", operand_type);
    c->whisper_ops = operand_type;
    c->resid16 = operand_type == PCE_OPERANDS_F16_RESID16;
    return PCE_OK;
}
int pce_whisper_get_operands(pce_ctx *c) { return c ? c->whisper_ops : PCE_E_INVALID; }

int pce_logmel_run(pce_ctx *c, int32_t n_mels) { return PCE_FWD(pce_logmel_run, c, n_mels); }
int pce_logmel_run_at(pce_ctx *c, int32_t n_mels, const int64_t *start_frames) { return PCE_FWD(pce_logmel_run_at, c, n_mels, start_frames); }
int pce_logmel_fetch(pce_ctx *c, int32_t clip, float *out) { return PCE_FWD(pce_logmel_fetch, c, clip, out); }
int pce_selftest_logmel_image(pce_ctx *c, int32_t clip, uint16_t *out) { return PCE_FWD(pce_selftest_logmel_image, c, clip, out); }
int pce_whisper_load(pce_ctx *c, const pce_whisper_dims *dims, const float *weights, int64_t n_floats) { return PCE_FWD(pce_whisper_load, c, dims, weights, n_floats); }
int pce_whisper_encode_run(pce_ctx *c) { return PCE_FWD(pce_whisper_encode_run, c); }
int pce_whisper_encode_fetch(pce_ctx *c, int32_t clip, float *out) { return PCE_FWD(pce_whisper_encode_fetch, c, clip, out); }
int pce_selftest_attention(pce_ctx *c, const uint16_t *q, const uint16_t *k, const uint16_t *v, int32_t clips, int32_t heads, int32_t q_len, int32_t k_len,
                           int32_t causal, int32_t mode, uint16_t *out, int32_t *fell_back)
{
    return PCE_FWD(pce_selftest_attention, c, q, k, v, clips, heads, q_len, k_len, causal, mode, out, fell_back);
}
int pce_selftest_attention_ragged(pce_ctx *c, const uint16_t *q, const uint16_t *k, const uint16_t *v, int32_t clips, int32_t heads, const int32_t *q_len,
                                  const int32_t *k_len, int32_t causal, int32_t mode, uint16_t *out, int64_t out_rows, int32_t *fell_back)
{
    return PCE_FWD(pce_selftest_attention_ragged, c, q, k, v, clips, heads, q_len, k_len, causal, mode, out, out_rows, fell_back);
}
int pce_selftest_attn1(pce_ctx *c, int32_t form, int32_t n, int32_t heads, const uint16_t *q, int64_t q_elems, uint16_t *k, int64_t k_elems, uint16_t *v,
                       int64_t v_elems, const int32_t *k_row0, const int32_t *len, const int32_t *skip, int32_t span, uint16_t *out, int64_t out_elems)
{
    return PCE_FWD(pce_selftest_attn1, c, form, n, heads, q, q_elems, k, k_elems, v, v_elems, k_row0, len, skip, span, out, out_elems);
}
int pce_selftest_align_matrix(pce_ctx *c, int32_t n, int32_t heads, const uint16_t *q, int64_t q_elems, const uint16_t *k, int64_t k_elems, int32_t k_rows,
                              const int32_t *t_len, const int32_t *f_len, const int32_t *heads_sel, int32_t n_sel, int32_t split, int32_t sot_len,
                              int32_t medfilt_width, float qk_scale, float *w_soft, int64_t w_soft_elems, float *w_norm, int64_t w_norm_elems, double *cost,
                              int64_t cost_elems)
{
    return PCE_FWD(pce_selftest_align_matrix, c, n, heads, q, q_elems, k, k_elems, k_rows, t_len, f_len, heads_sel, n_sel, split, sot_len, medfilt_width, qk_scale,
                   w_soft, w_soft_elems, w_norm, w_norm_elems, cost, cost_elems);
}
int pce_selftest_decode_rules(pce_ctx *c, int32_t form, int32_t n, int32_t n_vocab, int32_t steps, const float *logits, int64_t logits_elems, const int32_t *tokens,
                              const int32_t *token_offsets, int32_t pad_token, int32_t t_cap, const int32_t *sample_begin, int32_t sample_begin_all,
                              const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, int64_t mask_elems, float temperature, uint32_t seed_lo,
                              uint32_t seed_hi, int32_t probe_token, const int32_t *sample_keys, int32_t max_new, int32_t *out_tok, float *out_lp,
                              float *probe_prob, int64_t out_elems, int32_t *table, int64_t table_elems, int32_t *loop_state, int64_t state_elems)
{
    return PCE_FWD(pce_selftest_decode_rules, c, form, n, n_vocab, steps, logits, logits_elems, tokens, token_offsets, pad_token, t_cap, sample_begin, sample_begin_all,
                   rules, vocab_mask, mask_elems, temperature, seed_lo, seed_hi, probe_token, sample_keys, max_new, out_tok, out_lp, probe_prob, out_elems, table,
                   table_elems, loop_state, state_elems);
}
int pce_selftest_gemm(pce_ctx *c, const uint16_t *A, const uint16_t *B, const float *bias, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t rows_per_clip,
                      int32_t vt_sp, uint16_t *out)
{
    return PCE_FWD(pce_selftest_gemm, c, A, B, bias, M, N, K, epilogue, rows_per_clip, vt_sp, out);
}
int pce_selftest_gemm_resid(pce_ctx *c, const uint16_t *A, const uint16_t *B, const float *bias, uint16_t *resid_inout, int32_t M, int32_t N, int32_t K)
{
    return PCE_FWD(pce_selftest_gemm_resid, c, A, B, bias, resid_inout, M, N, K);
}
int pce_selftest_xattn(pce_ctx *c, const float *resid, const float *ln_w, const float *ln_b, const uint16_t *wq, const float *bq, const uint16_t *wk, const uint16_t *wv,
                       const float *bv, const uint16_t *E, const int32_t *k_len, int32_t n, int32_t k_cap, int32_t d, int32_t heads, int32_t workgroups_per_clip, uint16_t *out)
{
    return PCE_FWD(pce_selftest_xattn, c, resid, ln_w, ln_b, wq, bq, wk, wv, bv, E, k_len, n, k_cap, d, heads, workgroups_per_clip, out);
}
int pce_selftest_gemm_tiled(pce_ctx *c, int32_t kernel, int32_t epilogue, const uint16_t *A, int64_t a_len, int64_t lda, int64_t a_batch, int32_t batch,
                            const uint16_t *B, const float *bias, int32_t M, int32_t N, int32_t K, void *C, int64_t c_len, int64_t ldc, int64_t c_batch,
                            const float *pos, int32_t pos_T, int32_t v_col0, int32_t rows_per_clip, int32_t vt_sp, uint16_t *vt, int64_t vt_len, int32_t *kernel_used)
{
    return PCE_FWD(pce_selftest_gemm_tiled, c, kernel, epilogue, A, a_len, lda, a_batch, batch, B, bias, M, N, K, C, c_len, ldc, c_batch, pos, pos_T, v_col0,
                   rows_per_clip, vt_sp, vt, vt_len, kernel_used);
}
int pce_selftest_layernorm(pce_ctx *c, int32_t form, int32_t rows, int32_t d, const void *x, const uint16_t *delta, const uint16_t *delta2, const float *w,
                           const float *b, float eps, int32_t flags, void *out, void *resid_out, uint16_t *out_copy)
{
    return PCE_FWD(pce_selftest_layernorm, c, form, rows, d, x, delta, delta2, w, b, eps, flags, out, resid_out, out_copy);
}
int pce_whisper_decoder_load(pce_ctx *c, const pce_whisper_text_dims *dims, const float *weights, int64_t n_floats)
{
    return PCE_FWD(pce_whisper_decoder_load, c, dims, weights, n_floats);
}
int pce_whisper_align_run(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const int32_t *num_frames, int32_t sot_len, const uint8_t *head_mask,
                          int32_t medfilt_width, float qk_scale)
{
    return PCE_FWD(pce_whisper_align_run, c, tokens, token_offsets, num_frames, sot_len, head_mask, medfilt_width, qk_scale);
}
int pce_whisper_align_fetch(pce_ctx *c, int32_t clip, int32_t *text_idx, int32_t *time_idx, int32_t *path_len, double *cost)
{
    return PCE_FWD(pce_whisper_align_fetch, c, clip, text_idx, time_idx, path_len, cost);
}
int pce_whisper_align_shape(pce_ctx *c, int32_t clip, int32_t *n_rows, int32_t *n_cols) { return PCE_FWD(pce_whisper_align_shape, c, clip, n_rows, n_cols); }
int pce_whisper_align_paths_enqueue(pce_ctx *c, int32_t slot, int32_t *n_clips, int32_t *path_stride) { return PCE_FWD(pce_whisper_align_paths_enqueue, c, slot, n_clips, path_stride); }
int pce_whisper_align_paths_wait(pce_ctx *c, int32_t slot, int32_t *path_len, int32_t *text_idx, int32_t *time_idx)
{
    return PCE_FWD(pce_whisper_align_paths_wait, c, slot, path_len, text_idx, time_idx);
}
int pce_whisper_sample_keys(pce_ctx *c, const int32_t *keys, int32_t n) { return PCE_FWD(pce_whisper_sample_keys, c, keys, n); }
int pce_whisper_decode_step(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, int32_t sample_begin, const pce_whisper_decode_rules *rules,
                            const uint8_t *vocab_mask, int32_t *next_tokens, float *next_logprobs)
{
    return PCE_FWD(pce_whisper_decode_step, c, tokens, token_offsets, sample_begin, rules, vocab_mask, next_tokens, next_logprobs);
}
int pce_whisper_decode_step_ex(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask,
                               const pce_whisper_decode_opts *opts, int32_t *next_tokens, float *next_logprobs, float *probe_prob)
{
    return PCE_FWD(pce_whisper_decode_step_ex, c, tokens, token_offsets, rules, vocab_mask, opts, next_tokens, next_logprobs, probe_prob);
}
int pce_whisper_decode_loop(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask,
                            const pce_whisper_decode_opts *opts, int32_t max_new, int32_t check_every, int32_t *out_tokens, float *out_logprobs, int32_t *out_steps,
                            float *probe_prob)
{
    return PCE_FWD(pce_whisper_decode_loop, c, tokens, token_offsets, rules, vocab_mask, opts, max_new, check_every, out_tokens, out_logprobs, out_steps, probe_prob);
}
int pce_whisper_detect_language(pce_ctx *c, int32_t sot, int32_t lang_begin, int32_t n_lang, int32_t *ids, float *probs)
{
    return PCE_FWD(pce_whisper_detect_language, c, sot, lang_begin, n_lang, ids, probs);
}
int pce_bert_load(pce_ctx *c, const pce_bert_dims *dims, const float *weights, int64_t n_floats) { return PCE_FWD(pce_bert_load, c, dims, weights, n_floats); }
int pce_bert_run(pce_ctx *c, const int32_t *input_ids, const int32_t *offsets, int32_t n_seq) { return PCE_FWD(pce_bert_run, c, input_ids, offsets, n_seq); }
int pce_bert_fetch(pce_ctx *c, int32_t seq, float *logits, int32_t *labels) { return PCE_FWD(pce_bert_fetch, c, seq, logits, labels); }
// (the loader's conditions are the same in both operand builds)
int pce_w2v_check(const pce_w2v_dims *dims, int64_t n_floats, char *msg, size_t cap) { return pce_w2v_check_f16(dims, n_floats, msg, cap); }
int pce_w2v_load(pce_ctx *c, const pce_w2v_dims *dims, const float *weights, int64_t n_floats) { return PCE_FWD(pce_w2v_load, c, dims, weights, n_floats); }
int pce_w2v_run(pce_ctx *c, const pce_w2v_plan *plan) { return PCE_FWD(pce_w2v_run, c, plan); }
int pce_w2v_shape(pce_ctx *c, int32_t clip, int64_t *n_frames, int32_t *n_cols) { return PCE_FWD(pce_w2v_shape, c, clip, n_frames, n_cols); }
int pce_w2v_fetch(pce_ctx *c, int32_t clip, float *log_probs) { return PCE_FWD(pce_w2v_fetch, c, clip, log_probs); }
int pce_w2v_device(pce_ctx *c, const float **d_emissions, const int64_t **h_row_start, const int32_t **h_n_frames, int32_t *n_cols)
{
    return PCE_FWD(pce_w2v_device, c, d_emissions, h_row_start, h_n_frames, n_cols);
}
// windows and kept frames of one clip: ctc_emissions.window_plan's arithmetic (true division and truncation in double)
int pce_w2v_window_plan(int64_t n_samples, int32_t window_samples, int32_t context_samples, int64_t *n_windows, int64_t *n_frames)
{
    if (n_samples < 0 || window_samples < 1 || context_samples < 0 || !n_windows || !n_frames) return PCE_E_INVALID;
    const int64_t window = window_samples, n_win = n_samples > window ? (n_samples + window - 1) / window : 1, extension = n_win * window - n_samples;
    const int64_t wf = (int64_t)((double)window / 16000.0 * 50.0);
    *n_windows = n_win;
    *n_frames = n_win * wf - (extension > 0 ? (int64_t)((double)extension / 16000.0 * 50.0) : 0);
    return PCE_OK;
}
int pce_selftest_w2v_wave(pce_ctx *c, const int16_t *pcm, int64_t n_samples, int32_t window_samples, int32_t context_samples, int32_t feat_norm, int32_t C,
                          int32_t stride, const float *w, const float *bias, const float *gamma, const float *beta, uint16_t *out)
{
    return PCE_FWD(pce_selftest_w2v_wave, c, pcm, n_samples, window_samples, context_samples, feat_norm, C, stride, w, bias, gamma, beta, out);
}
int pce_selftest_w2v_lngelu(pce_ctx *c, const uint16_t *x, int32_t rows, int32_t C, const float *w, const float *b, float eps, int32_t gelu, uint16_t *out)
{
    return PCE_FWD(pce_selftest_w2v_lngelu, c, x, rows, C, w, b, eps, gelu, out);
}
int pce_selftest_w2v_posconv(pce_ctx *c, const float *x, int32_t n_win, int32_t T, int32_t d, int32_t groups, const uint16_t *w, const float *bias, float *out)
{
    return PCE_FWD(pce_selftest_w2v_posconv, c, x, n_win, T, d, groups, w, bias, out);
}

} // extern "C"
