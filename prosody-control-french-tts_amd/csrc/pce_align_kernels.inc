// pce_align_kernels.inc -- the alignment-matrix kernels of the forced alignment and their launchers (included by pce_whisper_impl.inc inside its
// anonymous namespace).
// softmax over the audio frames of the (scaled) cross-attention logits of one alignment head:
// w[clip][sel][t][s] = softmax_s(q_t . k_s * 0.125 * qk_scale), s < F_c.  16 tokens per workgroup, 4 waves x 16
// keys per 64-key tile on v_mfma_f32_16x16x32_bf16, two passes (row max / sum, then normalised write).
struct AlignArgs {
    const op_t *q; int64_t q_ld;             // decoder cross-attention queries [clips * T_pad][d]
    const op_t *k; int64_t k_ld;             // audio keys of this layer      [clips * 1500][d]
    const int *t_len, *f_len;                // per clip: tokens, frames considered (num_frames // 2)
    const int *heads;                        // head index of every selected head of this layer
    float *w; int sel0, n_sel_total, T_pad, F_pad;
    float scale;
};
__global__ __launch_bounds__(256) void k_align_scores(AlignArgs A)
{
    __shared__ float red_m[4][16], red_s[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int clip = blockIdx.z, sel = blockIdx.y, t0 = blockIdx.x * 16;
    const int T = A.t_len[clip], F = A.f_len[clip];
    if (t0 >= T || F <= 0) return;
    const int head = A.heads[sel];
    const op_t *qb = A.q + ((int64_t)clip * A.T_pad) * A.q_ld + head * 64;
    const op_t *kb = A.k + ((int64_t)clip * W_CTX) * A.k_ld + head * 64;
    opx8 qf[2];
    {
        int tr = t0 + fr; if (tr >= T) tr = T - 1;
        qf[0] = *reinterpret_cast<const opx8 *>(qb + (int64_t)tr * A.q_ld + fq * 8);
        qf[1] = *reinterpret_cast<const opx8 *>(qb + (int64_t)tr * A.q_ld + 32 + fq * 8);
    }
    float *wb = A.w + (((int64_t)clip * A.n_sel_total + A.sel0 + sel) * A.T_pad) * (int64_t)A.F_pad;
    float m_run[4], l_run[4];
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) { m_run[r4] = -1e30f; l_run[r4] = 0.f; }
    for (int pass = 0; pass < 2; pass++) {
        for (int s0 = wv * 16; s0 < F; s0 += 64) {
            int kr = s0 + fr; if (kr >= F) kr = F - 1;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; kk++) {
                const opx8 kf = *reinterpret_cast<const opx8 *>(kb + (int64_t)kr * A.k_ld + kk * 32 + fq * 8);
                acc = mfma16(qf[kk], kf, acc);
            }
            const bool valid = (s0 + fr) < F;                  // column = key s0 + fr, rows = tokens fq*4 + r4
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) {
                const float v = valid ? acc[r4] * A.scale : -1e30f;
                if (pass == 0) {
                    const float mx = dpp_row_max<16>(v);
                    const float m_new = fmaxf(m_run[r4], mx);
                    const float e = valid ? __expf(v - m_new) : 0.f;
                    l_run[r4] = l_run[r4] * __expf(m_run[r4] - m_new) + dpp_row_sum<16>(e);
                    m_run[r4] = m_new;
                } else if (valid && t0 + fq * 4 + r4 < T) {
                    wb[(int64_t)(t0 + fq * 4 + r4) * A.F_pad + s0 + fr] = __expf(v - m_run[r4]) / l_run[r4];
                }
            }
        }
        if (pass == 0) {                                       // merge the four waves' partial (max, sum) per token row
            if (fr == 0)
#pragma unroll
                for (int r4 = 0; r4 < 4; r4++) { red_m[wv][fq * 4 + r4] = m_run[r4]; red_s[wv][fq * 4 + r4] = l_run[r4]; }
            __syncthreads();
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) {
                const int row = fq * 4 + r4;
                float m = fmaxf(fmaxf(red_m[0][row], red_m[1][row]), fmaxf(red_m[2][row], red_m[3][row]));
                float l = 0.f;
                for (int u = 0; u < 4; u++) l += red_s[u][row] * __expf(red_m[u][row] - m);
                m_run[r4] = m; l_run[r4] = l;
            }
        }
    }
}

// std/mean normalisation over the token axis (torch.std_mean(dim=-2, unbiased=False)), in place
__global__ __launch_bounds__(256) void k_align_colnorm(float *__restrict__ w, const int *__restrict__ t_len, const int *__restrict__ f_len,
                                                      int n_sel, int T_pad, int F_pad)
{
    const int clip = blockIdx.z, sel = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
    const int T = t_len[clip], F = f_len[clip];
    if (s >= F) return;
    float *col = w + (((int64_t)clip * n_sel + sel) * T_pad) * (int64_t)F_pad + s;
    if (T <= 64) {                                               // the usual case (a window's tokens): the column lives in registers, one read and one write
        float v[64];
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 64; t++) { v[t] = t < T ? __builtin_nontemporal_load(col + (int64_t)t * F_pad) : 0.f; sum += v[t]; }      // (same order of additions as the loop below)
        const float mean = sum / (float)T;
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < 64; t++) if (t < T) { const float a = v[t] - mean; q += a * a; }
        const float sd = sqrtf(q / (float)T);
#pragma unroll
        for (int t = 0; t < 64; t++) if (t < T) col[(int64_t)t * F_pad] = (v[t] - mean) / sd;
        return;
    }
    float sum = 0.f;
    for (int t = 0; t < T; t++) sum += col[(int64_t)t * F_pad];
    const float mean = sum / (float)T;
    float q = 0.f;
    for (int t = 0; t < T; t++) { const float a = col[(int64_t)t * F_pad] - mean; q += a * a; }
    const float sd = sqrtf(q / (float)T);
    for (int t = 0; t < T; t++) col[(int64_t)t * F_pad] = (col[(int64_t)t * F_pad] - mean) / sd;
}

// median filter along time (reflect padding), mean over the selected heads, rows [sot_len, T-1) -> cost = -mean (fp64).
// WIDTH 7 (whisper-timestamped's default) selects with a 13-exchange network in registers; WIDTH 0 is the generic
// insertion sort (<= 15 taps, a scratch array: 20 x slower, measured 6.1 ms vs 0.3 ms per 256 clips).
__device__ __forceinline__ void cswap(float &a, float &b) { const bool sw = a > b; const float lo = sw ? b : a, hi = sw ? a : b; a = lo; b = hi; }
template <int WIDTH>
__global__ __launch_bounds__(256) void k_align_cost(const float *__restrict__ w, const int *__restrict__ t_len, const int *__restrict__ f_len,
                                                   int n_sel, int T_pad, int F_pad, int sot_len, int width, int N_max,
                                                   double *__restrict__ cost /* [clips][N_max][F_pad] */)
{
    const int clip = blockIdx.z, row = blockIdx.y, s = blockIdx.x * blockDim.x + threadIdx.x;
    const int T = t_len[clip], F = f_len[clip];
    const int t = row + sot_len;
    if (t >= T - 1 || s >= F) return;
    const int pad = width / 2;
    float acc = 0.f;
    if (WIDTH == 7 && F > 3) {
        int idx[7];
#pragma unroll
        for (int u = 0; u < 7; u++) {
            int i = s - 3 + u;
            if (i < 0) i = -i;
            if (i >= F) i = 2 * (F - 1) - i;
            idx[u] = i;
        }
        for (int sel = 0; sel < n_sel; sel++) {
            const float *rp = w + ((((int64_t)clip * n_sel + sel) * T_pad) + t) * (int64_t)F_pad;
            float p0 = rp[idx[0]], p1 = rp[idx[1]], p2 = rp[idx[2]], p3 = rp[idx[3]], p4 = rp[idx[4]], p5 = rp[idx[5]], p6 = rp[idx[6]];
            cswap(p0, p5); cswap(p0, p3); cswap(p1, p6); cswap(p2, p4); cswap(p0, p1); cswap(p3, p5); cswap(p2, p6);
            cswap(p2, p3); cswap(p3, p6); cswap(p4, p5); cswap(p1, p4); cswap(p1, p3); cswap(p3, p4);
            acc += p3;
        }
    } else {
        for (int sel = 0; sel < n_sel; sel++) {
            const float *rp = w + ((((int64_t)clip * n_sel + sel) * T_pad) + t) * (int64_t)F_pad;
            float v;
            if (F <= pad) v = rp[s];                               // torch skips the filter for very short rows
            else {
                float win[15];
                for (int u = 0; u < width; u++) {
                    int idx = s - pad + u;
                    if (idx < 0) idx = -idx;
                    if (idx >= F) idx = 2 * (F - 1) - idx;
                    win[u] = rp[idx];
                }
                for (int a = 1; a < width; a++) {                  // insertion sort of <= 15 values
                    const float key = win[a]; int b = a - 1;
                    while (b >= 0 && win[b] > key) { win[b + 1] = win[b]; b--; }
                    win[b + 1] = key;
                }
                v = win[pad];
            }
            acc += v;
        }
    }
    cost[((int64_t)clip * N_max + row) * F_pad + s] = -(double)(acc / (float)n_sel);
}

// ---- The forced alignment's matrix, as pce_whisper_align_run and pce_selftest_align_matrix (its test hook) build it: shapes, then the three launches.
// Per clip: T tokens (sot_len + 2 .. T_cap), F frames (1 .. 1500); `dims` keeps the running maxima (F_max, N_max = the DTW's rows of the longest clip).
static int token_rows_pad(int T_max) { return (int)div_up(T_max, 16) * 16; }            // an MFMA row block is 16 rows
struct AlignDims { int F_max = 0, N_max = 0; int F_pad() const { return (int)div_up(F_max, 64) * 64; } };
static bool align_width_ok(int width) { return width >= 1 && width <= 15 && (width & 1); }
static int align_clip_dims(pce_ctx *c, int clip, int T, int F, int sot_len, int T_cap, AlignDims &dims)
{
    if (T < sot_len + 2 || T > T_cap) return pce_fail(c, PCE_E_INVALID, "clip %d: %d tokens (need %d..%d)", clip, T, sot_len + 2, T_cap);
    if (F < 1) return pce_fail(c, PCE_E_INVALID, "clip %d: no audio frames", clip);
    dims.F_max = std::max(dims.F_max, F); dims.N_max = std::max(dims.N_max, T - sot_len - 1);
    return PCE_OK;
}
// the weights w [n][n_sel][T_pad][F_pad] with the per-clip lengths on the device
struct AlignMatrix { float *w; const int *t_len, *f_len; int n, n_sel, T_pad, F_pad; };
// one layer's scores: its ns selected heads heads[sel0 .. sel0 + ns) fill slices sel0 .. of w; q [n * T_pad][d], k [n * 1500][d]
static void launch_align_scores(pce_ctx *c, const AlignMatrix &m, const op_t *q, const op_t *k, int d, const int *heads, int sel0, int ns, float qk_scale)
{
    AlignArgs g{};
    g.q = q; g.q_ld = d; g.k = k; g.k_ld = d; g.t_len = m.t_len; g.f_len = m.f_len;
    g.heads = heads + sel0;
    g.w = m.w; g.sel0 = sel0; g.n_sel_total = m.n_sel; g.T_pad = m.T_pad; g.F_pad = m.F_pad;
    g.scale = 0.125f * qk_scale;
    hipLaunchKernelGGL(k_align_scores, dim3((unsigned)div_up(m.T_pad, 16), (unsigned)ns, (unsigned)m.n), dim3(256), 0, c->stream, g);
}
// normalise over tokens (in place), then median filter over time, mean over heads -> cost [n][N_max][F_pad]
static void launch_align_cost(pce_ctx *c, const AlignMatrix &m, int sot_len, int medfilt_width, int N_max, double *cost)
{
    hipLaunchKernelGGL(k_align_colnorm, dim3((unsigned)div_up(m.F_pad, 256), (unsigned)m.n_sel, (unsigned)m.n), dim3(256), 0, c->stream,
                       m.w, m.t_len, m.f_len, m.n_sel, m.T_pad, m.F_pad);
    if (medfilt_width == 7 && !c->sw.generic_median)
        hipLaunchKernelGGL((k_align_cost<7>), dim3((unsigned)div_up(m.F_pad, 256), (unsigned)N_max, (unsigned)m.n), dim3(256), 0, c->stream,
                           m.w, m.t_len, m.f_len, m.n_sel, m.T_pad, m.F_pad, sot_len, medfilt_width, N_max, cost);
    else
        hipLaunchKernelGGL((k_align_cost<0>), dim3((unsigned)div_up(m.F_pad, 256), (unsigned)N_max, (unsigned)m.n), dim3(256), 0, c->stream,
                           m.w, m.t_len, m.f_len, m.n_sel, m.T_pad, m.F_pad, sot_len, medfilt_width, N_max, cost);
}
