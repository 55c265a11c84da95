// pce_decode_rules.inc -- the token choice of a decoding step: k_decode_rules, k_step_advance and the language probe k_lang_probs (included by
// pce_whisper_impl.inc inside its anonymous namespace).
// openai-whisper decoding.py at temperature 0, one workgroup per sequence: SuppressBlank, SuppressTokens,
// ApplyTimestampRules on the logits of the last position, then the GreedyDecoder's arg-max (first maximum) and its
// "once end-of-text, always end-of-text" rule.  vmask: bit 0 = always suppressed (suppress list, no_timestamps),
// bit 1 = suppressed at the first sampled position (blank, end of text).
struct DecRules { int eot, ts_begin, n_vocab, ld, sample_begin, max_initial_ts; float temperature; unsigned seed_lo, seed_hi; int probe; };
// uniform in (0, 1) from (seed, clip, position, token): two rounds of the splitmix64 finaliser over the packed counter
__device__ __forceinline__ float dec_uniform(unsigned seed_lo, unsigned seed_hi, int clip, int pos, int v)
{
    unsigned long long z = ((unsigned long long)seed_hi << 32 | seed_lo) + 0x9E3779B97F4A7C15ull * ((unsigned long long)(unsigned)clip << 40 ^ (unsigned long long)(unsigned)pos << 20 ^ (unsigned)v);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    // 23 random bits + 1/2: every value is exact in float and lies strictly inside (0, 1) (24 bits + 1/2 rounds to 1.0 at the top)
    return ((float)(unsigned)(z >> 41) + 0.5f) * (1.0f / 8388608.0f);
}
// DR_T threads: the kernel is one workgroup per sequence making five passes over its 50 000 logits (L2-resident); with 256 threads each pass
// was ~200 dependent-looking iterations per thread and the launch took 183 us for 256 sequences; 1 024 threads keep four times the loads in flight
constexpr int DR_T = 1024, DR_W = DR_T / 64, DR_K = 51;      // DR_K ids per thread: vocabularies up to 52 224 (the multilingual 51 865, large-v3's 51 866)
__device__ __forceinline__ float dr_max(const float *r) { float m = r[0];
#pragma unroll
    for (int u = 1; u < DR_W; u++) m = fmaxf(m, r[u]);
    return m; }
__device__ __forceinline__ float dr_sum(const float *r) { float m = 0.f;
#pragma unroll
    for (int u = 0; u < DR_W; u++) m += r[u];
    return m; }
__global__ __launch_bounds__(DR_T) void k_decode_rules(const float *__restrict__ logits, const int *__restrict__ tokens, const int *__restrict__ t_len,
                                                     int T_pad, const unsigned char *__restrict__ vmask, DecRules R, const int *__restrict__ sample_begin_of,
                                                     int *__restrict__ next, float *__restrict__ next_logprob, float *__restrict__ probe_prob,
                                                     const int *__restrict__ sample_key)
{
    __shared__ float r_f[2][DR_W]; __shared__ int r_i[DR_W]; __shared__ float s_bcast[2]; __shared__ int s_flags[4];
    const int clip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = t_len[clip];
    const int *seq = tokens + (size_t)clip * T_pad;
    const float *x = logits + (size_t)clip * R.ld;
    if (sample_begin_of) R.sample_begin = sample_begin_of[clip];
    // The row lives in REGISTERS from here on (thread t owns ids t, t + 1024, ...: DR_K of them): one read of the logits instead of one per pass and a
    // write-back nobody read (round 5: 69 -> ~25 us per launch; the loops visit the same ids in the same order per thread: the same bits)
    float xr[DR_K];
#pragma unroll
    for (int k = 0; k < DR_K; k++) { const int v = tid + k * DR_T; xr[k] = v < R.n_vocab ? x[v] : 0.f; }
    if (R.probe >= 0 && probe_prob) {
        // softmax of the unfiltered logits at one token (no_speech_prob when the prefix ends at <|startoftranscript|>)
        float m = -__builtin_huge_valf();
#pragma unroll
        for (int k = 0; k < DR_K; k++) if (tid + k * DR_T < R.n_vocab) m = fmaxf(m, xr[k]);
        m = wave_xor_max(m);
        if (lane == 0) r_f[0][wv] = m;
        __syncthreads();
        m = dr_max(r_f[0]);
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < DR_K; k++) if (tid + k * DR_T < R.n_vocab) se += __expf(xr[k] - m);
        se = wave_xor_sum(se);
        if (lane == 0) r_f[1][wv] = se;
        __syncthreads();
        if (tid == 0) probe_prob[clip] = __expf(x[R.probe] - m) / dr_sum(r_f[1]);
        __syncthreads();
    }
    if (tid == 0) {
        const int ns = L - R.sample_begin;                         // sampled tokens so far
        const bool last_ts = ns >= 1 && seq[L - 1] >= R.ts_begin;
        const bool pen_ts = ns < 2 || seq[L - 2] >= R.ts_begin;
        int last_stamp = -1;
        for (int t = R.sample_begin; t < L; t++) if (seq[t] >= R.ts_begin) last_stamp = seq[t];
        int ts_floor = R.ts_begin;                                 // timestamps below this are forbidden
        if (last_stamp >= 0) ts_floor = (last_ts && !pen_ts) ? last_stamp : last_stamp + 1;
        s_flags[0] = last_ts ? (pen_ts ? 1 : 2) : 0;               // 1: no timestamp may follow, 2: no text token may follow
        s_flags[1] = ts_floor;
        s_flags[2] = ns == 0;
        s_flags[3] = L > 0 && seq[L - 1] == R.eot;
    }
    __syncthreads();
    const int pair = s_flags[0], ts_floor = s_flags[1]; const bool first = s_flags[2] != 0, done = s_flags[3] != 0;
    const float NEG = -__builtin_huge_valf();
    // pass 1: masks; maximum over the text ids and over the timestamp ids
    float m_text = NEG, m_ts = NEG;
#pragma unroll
    for (int k = 0; k < DR_K; k++) {
        const int v = tid + k * DR_T;
        if (v >= R.n_vocab) break;
        float a = xr[k];
        const unsigned char mk = vmask[v];
        bool off = (mk & 1) || (first && (mk & 2));
        if (pair == 1 && v >= R.ts_begin) off = true;
        if (pair == 2 && v < R.eot) off = true;
        if (v >= R.ts_begin && v < ts_floor) off = true;
        if (first && (v < R.ts_begin || (R.max_initial_ts >= 0 && v > R.ts_begin + R.max_initial_ts))) off = true;
        if (off) a = NEG;
        xr[k] = a;
        if (v < R.ts_begin) m_text = fmaxf(m_text, a); else m_ts = fmaxf(m_ts, a);
    }
    m_text = wave_xor_max(m_text); m_ts = wave_xor_max(m_ts);
    if (lane == 0) { r_f[0][wv] = m_text; r_f[1][wv] = m_ts; }
    __syncthreads();
    m_text = dr_max(r_f[0]);
    m_ts = dr_max(r_f[1]);
    __syncthreads();
    // pass 2: log-sum-exp over the timestamps; "if the probability mass of the timestamps exceeds every text token, sample a timestamp"
    float se = 0.f;
    if (m_ts > NEG) {
        // (the timestamps start at ts_begin: the thread that the old loop's first id ts_begin + t fell on is (ts_begin + t) mod 1024, so the per-thread
        //  sums regroup -- the ids of a thread are still visited in ascending order; the total differs from the round-4 kernel's in the last bits only)
#pragma unroll
        for (int k = 0; k < DR_K; k++) { const int v = tid + k * DR_T; if (v >= R.ts_begin && v < R.n_vocab) se += __expf(xr[k] - m_ts); }
    }
    se = wave_xor_sum(se);
    if (lane == 0) r_f[0][wv] = se;
    __syncthreads();
    if (tid == 0) {
        const float tot = dr_sum(r_f[0]);
        const float lse_ts = m_ts > NEG ? m_ts + __logf(tot) : NEG;
        s_bcast[0] = (lse_ts > m_text) ? 1.f : 0.f;
    }
    __syncthreads();
    const bool only_ts = s_bcast[0] != 0.f;
    // pass 3: arg-max (first maximum); at a temperature the arg-max of logits / temperature + Gumbel noise, which is one
    // draw from softmax(logits / temperature) (Categorical(logits = logits / temperature).sample() of GreedyDecoder.update)
    float best = NEG; int bi = 0x7fffffff;
    const bool sampling = R.temperature > 0.f;
    const int draw_key = sample_key ? sample_key[clip] : clip;      // (what the noise is keyed by: the caller's id of the clip, else its batch position)
    const float inv_t = sampling ? 1.0f / R.temperature : 1.0f;
    const int v_lo = only_ts ? R.ts_begin : 0;
#pragma unroll
    for (int k = 0; k < DR_K; k++) {
        const int v = tid + k * DR_T;
        if (v < v_lo || v >= R.n_vocab) continue;
        float a = xr[k];
        if (sampling && a > NEG) a = a * inv_t - __logf(-__logf(dec_uniform(R.seed_lo, R.seed_hi, draw_key, L, v)));
        if (a > best) { best = a; bi = v; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { r_f[0][wv] = best; r_i[wv] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int u = 1; u < DR_W; u++) if (r_f[0][u] > best || (r_f[0][u] == best && r_i[u] < bi)) { best = r_f[0][u]; bi = r_i[u]; }
        if (bi == 0x7fffffff) bi = only_ts ? R.ts_begin : 0;       // every candidate is -inf: torch.argmax returns the first index
        next[clip] = done ? R.eot : bi;
        s_bcast[1] = best; s_flags[0] = bi;
    }
    __syncthreads();
    if (sampling) {                                                // the choice's own (filtered, unscaled) logit: with its owner
        const int bi = s_flags[0];
        if ((bi & (DR_T - 1)) == tid) {
            float a = NEG;
#pragma unroll
            for (int k = 0; k < DR_K; k++) if (k == (bi >> 10)) a = xr[k];
            s_bcast[1] = a;
        }
        __syncthreads();
    }
    // log-probability of the choice under the filtered distribution (GreedyDecoder.update adds it to sum_logprobs unless
    // the sequence had already ended): log_softmax over what is left after the filters
    {
        const float top = s_bcast[1];                              // (a sampled choice need not be the maximum: exp(x - top) may exceed 1, the sum stays exact enough in float)
        float se2 = 0.f;
        if (top > NEG) {
#pragma unroll
            for (int k = 0; k < DR_K; k++) { const int v = tid + k * DR_T; if (v >= v_lo && v < R.n_vocab) se2 += __expf(xr[k] - top); }
        }
        se2 = wave_xor_sum(se2);
        __syncthreads();
        if (lane == 0) r_f[1][wv] = se2;
        __syncthreads();
        if (tid == 0) {
            const float tot = dr_sum(r_f[1]);
            next_logprob[clip] = (done || !(top > NEG)) ? 0.f : -__logf(tot);     // x[best] - logsumexp = -log(sum exp(x - best))
        }
    }
}

// openai-whisper decoding.py detect_language on the hidden state of the <|startoftranscript|> position, one workgroup per clip: the logits of the
// n_lang language tokens alone (rows lang_begin .. lang_begin + n_lang - 1 of the tied embedding: 99 or 100 rows of the 51 865 the output projection
// multiplies), their softmax -- every other token is masked to -inf there, so it is the softmax over the vocabulary -- and the arg-max, first maximum.
// Waves take rows (w, w + LANG_W, ...), the lanes of a wave split the width in runs of 8 operands (16-byte loads; column = 8 lane + 512 j), fp32
// accumulation in ascending column order per lane, the 64 partial sums added by xor shuffles 32 .. 1; wave 0 then holds logits i and i + 64 in lane i.
// The order of every addition follows from (d, n_lang) alone: a clip's results do not depend on what it is batched with, and two identical embedding
// rows give identical bits.  d: a multiple of 8, at most LN_D_MAX (pce_whisper_decoder_load: a multiple of 128).
constexpr int LANG_MAX = 128, LANG_T = 512, LANG_W = LANG_T / 64;
__global__ __launch_bounds__(LANG_T) void k_lang_probs(const op_t *__restrict__ hidden, const op_t *__restrict__ emb, int d, int lang_begin, int n_lang,
                                                       float *__restrict__ probs, int *__restrict__ ids)
{
    __shared__ float s_x[LN_D_MAX];
    __shared__ float s_logit[LANG_MAX];
    const int clip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const op_t *x = hidden + (int64_t)clip * d;
    for (int col = tid; col < d; col += LANG_T) s_x[col] = (float)x[col];
    __syncthreads();
    for (int r = wv; r < n_lang; r += LANG_W) {                    // (n_lang is no multiple of the wave count: the last round is short)
        const op_t *row = emb + (int64_t)(lang_begin + r) * d;
        float acc = 0.f;
        for (int col = lane * 8; col < d; col += 512) {            // (d is no multiple of 512 either: the high lanes sit out the last round, or every round)
            const opx8 e = *reinterpret_cast<const opx8 *>(row + col);
#pragma unroll
            for (int u = 0; u < 8; u++) acc = fmaf((float)e[u], s_x[col + u], acc);
        }
        acc = wave_xor_sum(acc);
        if (lane == 0) s_logit[r] = acc;
    }
    __syncthreads();
    if (wv != 0) return;
    const float NEG = -__builtin_huge_valf();
    const float a0 = lane < n_lang ? s_logit[lane] : NEG, a1 = lane + 64 < n_lang ? s_logit[lane + 64] : NEG;
    float best = a0; int bi = lane;                                // (lane 0 always holds a real logit: n_lang >= 1)
    if (a1 > best) { best = a1; bi = lane + 64; }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    const float e0 = lane < n_lang ? expf(a0 - best) : 0.f, e1 = lane + 64 < n_lang ? expf(a1 - best) : 0.f;
    float sum = e0 + e1;
    sum = wave_xor_sum(sum);
    float *p = probs + (int64_t)clip * n_lang;
    if (lane < n_lang) p[lane] = e0 / sum;
    if (lane + 64 < n_lang) p[lane + 64] = e1 / sum;
    if (lane == 0) ids[clip] = lang_begin + bi;
}
