// pce_whisper_entries.h -- the entry points of include/pce.h that take a context and exist once per operand build of the Whisper / BERT / wav2vec2
// unit (pce_whisper_bf16.hip, pce_whisper_f16.hip): X(name, (parameters), (arguments)), one line each.
//   * pce_whisper_impl.inc declares the table inside the build's namespace (pce_bf16 / pce_f16); it and the .inc files define the functions there;
//   * pce_whisper_dispatch.hip declares it inside both namespaces and generates the exported extern "C" function of every line, which forwards
//     to the build the context has selected.
// A line that disagrees with include/pce.h does not compile (conflicting extern "C" declaration), one that disagrees with a definition does not link.
// Not here (hand-written in pce_whisper_dispatch.hip): pce_whisper_set_operands / _get_operands, pce_w2v_window_plan, pce_w2v_segment_frames, pce_w2v_check (no context:
// always the fp16 build's) and pce_whisper_free.
#pragma once

#define PCE_DECLARE(name, params, args) int name params;

#define PCE_WHISPER_ENTRIES(X) \
    X(pce_logmel_run, (pce_ctx *c, int32_t n_mels), (c, n_mels)) \
    X(pce_logmel_run_at, (pce_ctx *c, int32_t n_mels, const int64_t *start_frames), (c, n_mels, start_frames)) \
    X(pce_logmel_fetch, (pce_ctx *c, int32_t clip, float *out), (c, clip, out)) \
    X(pce_selftest_logmel_image, (pce_ctx *c, int32_t clip, uint16_t *out), (c, clip, out)) \
    X(pce_whisper_load, (pce_ctx *c, const pce_whisper_dims *dims, const float *weights, int64_t n_floats), (c, dims, weights, n_floats)) \
    X(pce_whisper_encode_run, (pce_ctx *c), (c)) \
    X(pce_whisper_encode_fetch, (pce_ctx *c, int32_t clip, float *out), (c, clip, out)) \
    X(pce_selftest_attention, \
      (pce_ctx *c, const uint16_t *q, const uint16_t *k, const uint16_t *v, int32_t clips, int32_t heads, int32_t q_len, int32_t k_len, int32_t causal, \
       int32_t mode, uint16_t *out, int32_t *fell_back), \
      (c, q, k, v, clips, heads, q_len, k_len, causal, mode, out, fell_back)) \
    X(pce_selftest_attention_ragged, \
      (pce_ctx *c, const uint16_t *q, const uint16_t *k, const uint16_t *v, int32_t clips, int32_t heads, const int32_t *q_len, const int32_t *k_len, \
       int32_t causal, int32_t mode, uint16_t *out, int64_t out_rows, int32_t *fell_back), \
      (c, q, k, v, clips, heads, q_len, k_len, causal, mode, out, out_rows, fell_back)) \
    X(pce_selftest_attn1, \
      (pce_ctx *c, int32_t form, int32_t n, int32_t heads, const uint16_t *q, int64_t q_elems, uint16_t *k, int64_t k_elems, uint16_t *v, int64_t v_elems, \
       const int32_t *k_row0, const int32_t *len, const int32_t *skip, int32_t span, uint16_t *out, int64_t out_elems), \
      (c, form, n, heads, q, q_elems, k, k_elems, v, v_elems, k_row0, len, skip, span, out, out_elems)) \
    X(pce_selftest_align_matrix, \
      (pce_ctx *c, int32_t n, int32_t heads, const uint16_t *q, int64_t q_elems, const uint16_t *k, int64_t k_elems, int32_t k_rows, const int32_t *t_len, \
       const int32_t *f_len, const int32_t *heads_sel, int32_t n_sel, int32_t split, int32_t sot_len, int32_t medfilt_width, float qk_scale, float *w_soft, \
       int64_t w_soft_elems, float *w_norm, int64_t w_norm_elems, double *cost, int64_t cost_elems), \
      (c, n, heads, q, q_elems, k, k_elems, k_rows, t_len, f_len, heads_sel, n_sel, split, sot_len, medfilt_width, qk_scale, w_soft, w_soft_elems, w_norm, \
       w_norm_elems, cost, cost_elems)) \
    X(pce_selftest_decode_rules, \
      (pce_ctx *c, int32_t form, int32_t n, int32_t n_vocab, int32_t steps, const float *logits, int64_t logits_elems, const int32_t *tokens, \
       const int32_t *token_offsets, int32_t pad_token, int32_t t_cap, const int32_t *sample_begin, int32_t sample_begin_all, \
       const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, int64_t mask_elems, float temperature, uint32_t seed_lo, uint32_t seed_hi, \
       int32_t probe_token, const int32_t *sample_keys, int32_t max_new, int32_t *out_tok, float *out_lp, float *probe_prob, int64_t out_elems, int32_t *table, \
       int64_t table_elems, int32_t *loop_state, int64_t state_elems), \
      (c, form, n, n_vocab, steps, logits, logits_elems, tokens, token_offsets, pad_token, t_cap, sample_begin, sample_begin_all, rules, vocab_mask, mask_elems, \
       temperature, seed_lo, seed_hi, probe_token, sample_keys, max_new, out_tok, out_lp, probe_prob, out_elems, table, table_elems, loop_state, state_elems)) \
    X(pce_selftest_gemm, \
      (pce_ctx *c, const uint16_t *A, const uint16_t *B, const float *bias, int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t rows_per_clip, \
       int32_t vt_sp, uint16_t *out), \
      (c, A, B, bias, M, N, K, epilogue, rows_per_clip, vt_sp, out)) \
    X(pce_selftest_gemm_resid, \
      (pce_ctx *c, const uint16_t *A, const uint16_t *B, const float *bias, uint16_t *resid_inout, int32_t M, int32_t N, int32_t K), \
      (c, A, B, bias, resid_inout, M, N, K)) \
    X(pce_selftest_xattn, \
      (pce_ctx *c, const float *resid, const float *ln_w, const float *ln_b, const uint16_t *wq, const float *bq, const uint16_t *wk, const uint16_t *wv, \
       const float *bv, const uint16_t *E, const int32_t *k_len, int32_t n, int32_t k_cap, int32_t d, int32_t heads, int32_t workgroups_per_clip, uint16_t *out), \
      (c, resid, ln_w, ln_b, wq, bq, wk, wv, bv, E, k_len, n, k_cap, d, heads, workgroups_per_clip, out)) \
    X(pce_selftest_xattn_stages, \
      (pce_ctx *c, const float *resid, const float *ln_w, const float *ln_b, const uint16_t *wq, const float *bq, const uint16_t *wk, const uint16_t *wv, \
       const float *bv, const uint16_t *E, int64_t e_elems, const int32_t *k_len, const int32_t *skip, int32_t n, int32_t k_cap, int32_t d, int32_t heads, \
       int32_t workgroups_per_clip, uint16_t *out, int64_t out_elems, uint16_t *qp_hi, uint16_t *qp_lo, int64_t qp_elems, float *u_part, int64_t u_elems, \
       float *ml_part, int64_t ml_elems, int32_t *nodes_out), \
      (c, resid, ln_w, ln_b, wq, bq, wk, wv, bv, E, e_elems, k_len, skip, n, k_cap, d, heads, workgroups_per_clip, out, out_elems, qp_hi, qp_lo, qp_elems, \
       u_part, u_elems, ml_part, ml_elems, nodes_out)) \
    X(pce_selftest_gemm_tiled, \
      (pce_ctx *c, int32_t kernel, int32_t epilogue, const uint16_t *A, int64_t a_len, int64_t lda, int64_t a_batch, int32_t batch, const uint16_t *B, \
       const float *bias, int32_t M, int32_t N, int32_t K, void *C, int64_t c_len, int64_t ldc, int64_t c_batch, const float *pos, int32_t pos_T, \
       int32_t v_col0, int32_t rows_per_clip, int32_t vt_sp, uint16_t *vt, int64_t vt_len, int32_t *kernel_used), \
      (c, kernel, epilogue, A, a_len, lda, a_batch, batch, B, bias, M, N, K, C, c_len, ldc, c_batch, pos, pos_T, v_col0, rows_per_clip, vt_sp, vt, vt_len, \
       kernel_used)) \
    X(pce_selftest_layernorm, \
      (pce_ctx *c, int32_t form, int32_t rows, int32_t d, const void *x, const uint16_t *delta, const uint16_t *delta2, const float *w, const float *b, \
       float eps, int32_t flags, void *out, void *resid_out, uint16_t *out_copy), \
      (c, form, rows, d, x, delta, delta2, w, b, eps, flags, out, resid_out, out_copy)) \
    X(pce_selftest_encoder_walk, \
      (pce_ctx *c, int32_t pre_ln, int32_t gemm_rule, int32_t key_bias, int32_t d, int32_t heads, int32_t inner, int32_t n_layers, int32_t n_items, \
       int32_t rows_per_item, int32_t vt_sp, const int32_t *len, float eps, const float *weights, int64_t n_floats, const float *stream, int64_t stream_elems, \
       const uint16_t *ln_in, uint16_t *ln16, int64_t ln16_elems, uint16_t *qk, int64_t qk_elems, uint16_t *vt, int64_t vt_elems, uint16_t *attn, \
       int64_t attn_elems, uint16_t *hidden, int64_t hidden_elems, float *x32, int64_t x32_elems, int32_t *fit_out), \
      (c, pre_ln, gemm_rule, key_bias, d, heads, inner, n_layers, n_items, rows_per_item, vt_sp, len, eps, weights, n_floats, stream, stream_elems, ln_in, ln16, \
       ln16_elems, qk, qk_elems, vt, vt_elems, attn, attn_elems, hidden, hidden_elems, x32, x32_elems, fit_out)) \
    X(pce_whisper_decoder_load, (pce_ctx *c, const pce_whisper_text_dims *dims, const float *weights, int64_t n_floats), (c, dims, weights, n_floats)) \
    X(pce_whisper_align_run, \
      (pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const int32_t *num_frames, int32_t sot_len, const uint8_t *head_mask, \
       int32_t medfilt_width, float qk_scale), \
      (c, tokens, token_offsets, num_frames, sot_len, head_mask, medfilt_width, qk_scale)) \
    X(pce_whisper_align_fetch, (pce_ctx *c, int32_t clip, int32_t *text_idx, int32_t *time_idx, int32_t *path_len, double *cost), \
      (c, clip, text_idx, time_idx, path_len, cost)) \
    X(pce_whisper_align_shape, (pce_ctx *c, int32_t clip, int32_t *n_rows, int32_t *n_cols), (c, clip, n_rows, n_cols)) \
    X(pce_whisper_align_paths_enqueue, (pce_ctx *c, int32_t slot, int32_t *n_clips, int32_t *path_stride), (c, slot, n_clips, path_stride)) \
    X(pce_whisper_align_paths_wait, (pce_ctx *c, int32_t slot, int32_t *path_len, int32_t *text_idx, int32_t *time_idx), \
      (c, slot, path_len, text_idx, time_idx)) \
    X(pce_whisper_sample_keys, (pce_ctx *c, const int32_t *keys, int32_t n), (c, keys, n)) \
    X(pce_whisper_decode_step, \
      (pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, int32_t sample_begin, const pce_whisper_decode_rules *rules, \
       const uint8_t *vocab_mask, int32_t *next_tokens, float *next_logprobs), \
      (c, tokens, token_offsets, sample_begin, rules, vocab_mask, next_tokens, next_logprobs)) \
    X(pce_whisper_decode_step_ex, \
      (pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, \
       const pce_whisper_decode_opts *opts, int32_t *next_tokens, float *next_logprobs, float *probe_prob), \
      (c, tokens, token_offsets, rules, vocab_mask, opts, next_tokens, next_logprobs, probe_prob)) \
    X(pce_whisper_decode_loop, \
      (pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules, const uint8_t *vocab_mask, \
       const pce_whisper_decode_opts *opts, int32_t max_new, int32_t check_every, int32_t *out_tokens, float *out_logprobs, int32_t *out_steps, \
       float *probe_prob), \
      (c, tokens, token_offsets, rules, vocab_mask, opts, max_new, check_every, out_tokens, out_logprobs, out_steps, probe_prob)) \
    X(pce_whisper_detect_language, (pce_ctx *c, int32_t sot, int32_t lang_begin, int32_t n_lang, int32_t *ids, float *probs), \
      (c, sot, lang_begin, n_lang, ids, probs)) \
    X(pce_bert_load, (pce_ctx *c, const pce_bert_dims *dims, const float *weights, int64_t n_floats), (c, dims, weights, n_floats)) \
    X(pce_bert_run, (pce_ctx *c, const int32_t *input_ids, const int32_t *offsets, int32_t n_seq), (c, input_ids, offsets, n_seq)) \
    X(pce_bert_fetch, (pce_ctx *c, int32_t seq, float *logits, int32_t *labels), (c, seq, logits, labels)) \
    X(pce_w2v_load, (pce_ctx *c, const pce_w2v_dims *dims, const float *weights, int64_t n_floats), (c, dims, weights, n_floats)) \
    X(pce_w2v_run, (pce_ctx *c, const pce_w2v_plan *plan), (c, plan)) \
    X(pce_w2v_run_segments, (pce_ctx *c, const pce_w2v_segment *segments, int32_t n_segments, const pce_w2v_seg_plan *plan), (c, segments, n_segments, plan)) \
    X(pce_w2v_segments_plan, (pce_ctx *c, int64_t *n_chunks, int64_t *rows_computed, int64_t *rows_valid), (c, n_chunks, rows_computed, rows_valid)) \
    X(pce_w2v_shape, (pce_ctx *c, int32_t clip, int64_t *n_frames, int32_t *n_cols), (c, clip, n_frames, n_cols)) \
    X(pce_w2v_fetch, (pce_ctx *c, int32_t clip, float *log_probs), (c, clip, log_probs)) \
    X(pce_w2v_device, (pce_ctx *c, const float **d_emissions, const int64_t **h_row_start, const int32_t **h_n_frames, int32_t *n_cols), \
      (c, d_emissions, h_row_start, h_n_frames, n_cols)) \
    X(pce_selftest_w2v_wave, \
      (pce_ctx *c, const int16_t *pcm, int64_t n_samples, int32_t window_samples, int32_t context_samples, int32_t feat_norm, int32_t C, int32_t stride, \
       const float *w, const float *bias, const float *gamma, const float *beta, uint16_t *out), \
      (c, pcm, n_samples, window_samples, context_samples, feat_norm, C, stride, w, bias, gamma, beta, out)) \
    X(pce_selftest_w2v_lngelu, \
      (pce_ctx *c, const uint16_t *x, int32_t rows, int32_t C, const float *w, const float *b, float eps, int32_t gelu, uint16_t *out), \
      (c, x, rows, C, w, b, eps, gelu, out)) \
    X(pce_selftest_w2v_posconv, \
      (pce_ctx *c, const float *x, int32_t n_win, int32_t T, int32_t d, int32_t groups, const uint16_t *w, const float *bias, float *out), \
      (c, x, n_win, T, d, groups, w, bias, out)) \
    X(pce_selftest_w2v_wave_segments, \
      (pce_ctx *c, const int16_t *pcm, int64_t n_samples, const int64_t *seg, int32_t n_seg, int32_t min_samples, int32_t feat_norm, int32_t C, int32_t stride, \
       const float *w, const float *bias, const float *gamma, const float *beta, uint16_t *out), \
      (c, pcm, n_samples, seg, n_seg, min_samples, feat_norm, C, stride, w, bias, gamma, beta, out)) \
    X(pce_selftest_w2v_posconv_segments, \
      (pce_ctx *c, const float *x, int32_t n_win, const int32_t *len, int32_t T, int32_t d, int32_t groups, const uint16_t *w, const float *bias, float *out), \
      (c, x, n_win, len, T, d, groups, w, bias, out))
