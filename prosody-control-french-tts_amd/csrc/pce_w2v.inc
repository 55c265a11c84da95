// pce_w2v.inc -- the wav2vec2 / MMS CTC acoustic model (transformers' Wav2Vec2ForCTC in eval mode) on the resident 16 kHz batch: the emissions
// pce_ctc_align reads in place.  Included by pce_whisper_impl.inc after pce_bert.inc: the transformer body and six of the seven feature-encoder
// convolutions run on that file's GEMM / attention / LayerNorm launchers.  New here: the waveform layer with its normalisation (k_w2v_wave_*), the
// LayerNorm (+ GELU) over 16-bit rows (k_w2v_ln16), the grouped 128-tap positional convolution on MFMA (k_w2v_posconv) and the log-softmax /
// context-cut / star-column tail (k_w2v_tail).
//
// A window is window + 2 context samples at stride window over the clip, `context` zeros in front and zeros behind to a whole number of windows
// (ctc-forced-aligner's generate_emissions, as Aligners/ctc_emissions.hf_emissions restates it).  The windows are never materialised: the
// waveform layer reads the resident PCM through a per-window table {first sample of the clip, the window's first sample relative to it, the
// clip's length} and supplies the zeros itself.  Every image is time-major, [window][frame][channel]; from the last convolution on a window's
// frames are padded to T_pad = 16 ceil(T / 16) rows (the transposed-V epilogue writes four frames at a time).  Pad rows hold finite values that
// no real row ever reads: GEMM rows are independent, the attention masks keys >= T, the positional convolution takes frames >= T as zeros.
// Which kernel computes a product follows from N and K alone (w2v_gemm), and no kernel reduces across windows: a window's emissions do not
// depend on the chunk size or on what the window is batched with.
//
// pce_w2v_run_segments runs the same model on segments of unequal length, each alone (whisperX's emissions); pce_w2v_seg_plan.h forms its
// chunks.  Both entries fill one description of a run (W2vRun) and share what follows (w2v_run_chunks, w2v_forward_chunk): every kernel that
// looks at an item's frame count reads it from a table, and equal windows are items whose counts are equal.
#include <cstdarg>
#include "pce_w2v_seg_plan.h"

namespace {

constexpr int WV_K0 = 10;              // taps of the waveform layer (every published wav2vec2 / MMS checkpoint)
constexpr int WV_STRIDE_MAX = 8;       // its stride, at most
constexpr int WV_PART = 1024;          // frames of one partial of the group-norm statistics (the fixed partition of the time axis)
constexpr int WV_TILE = 256;           // frames per workgroup of the group form's second pass
constexpr int WV_LN_F = 8;             // frames per workgroup of the layer form
constexpr int WV_C_MAX = 1024;         // channels of the waveform layer, at most (the layer form's LDS tile)
constexpr int PC_MT = 256, PC_TAPS = 128, PC_ROWS = PC_MT + PC_TAPS;      // positional convolution: frames per workgroup, taps, staged rows

typedef __attribute__((ext_vector_type(2))) op_t opx2;
typedef __attribute__((ext_vector_type(4))) op_t opx4_w;

__device__ __forceinline__ float w2v_sample(const int16_t *__restrict__ pcm, int64_t base, int64_t s0, int64_t n, int64_t i)
{
    const int64_t p = s0 + i;
    return (p >= 0 && p < n) ? (float)pcm[base + p] * (1.0f / 32768.0f) : 0.f;      // the zeros of the context and of the padding
}
// one output of the waveform convolution: the same operation sequence in the statistics pass and in the pass that recomputes it
__device__ __forceinline__ float w2v_conv10(const float *x, const float (&wk)[WV_K0], float b)
{
    float y = 0.f;
#pragma unroll
    for (int k = 0; k < WV_K0; k++) y = fmaf(x[k], wk[k], y);
    return y + b;
}

// The waveform layer's kernels and the positional convolution take every item's own frame count from a device table: a run over equal
// windows (pce_w2v_run) is a run over items whose counts are all the same.  A slot is the rows between two items' images: the chunk's longest
// item's frames.

// Group form, pass 1: sum and sum of squares of every channel over the frames [WV_PART p, WV_PART (p + 1)) of item blockIdx.y, in fp64.  The
// partition of the time axis is fixed, so an item has ceil(t0 / WV_PART) partials among the n_part slots of its row of `part`; a block behind
// its item's last frame leaves (the whole block: blockIdx decides)
__global__ __launch_bounds__(256) void k_w2v_wave_stats(const int16_t *__restrict__ pcm, const int64_t *__restrict__ win /* [W][3] */,
                                                        const float *__restrict__ w /* [C][10] */, const float *__restrict__ bias /* or null */, int C,
                                                        int stride, const int *__restrict__ t0 /* [W] */, int n_part,
                                                        double *__restrict__ part /* [W][n_part][2][C] */)
{
    const int T0 = t0[blockIdx.y];
    if ((int)blockIdx.x * WV_PART >= T0) return;
    __shared__ float xs[(WV_PART - 1) * WV_STRIDE_MAX + 16];
    const int wdx = (int)blockIdx.y, p = (int)blockIdx.x;
    const int64_t base = win[3 * wdx], s0 = win[3 * wdx + 1], n = win[3 * wdx + 2];
    const int f0 = p * WV_PART, nf = min(WV_PART, T0 - f0), ns = (nf - 1) * stride + WV_K0;
    for (int i = (int)threadIdx.x; i < ns; i += 256) xs[i] = w2v_sample(pcm, base, s0, n, (int64_t)f0 * stride + i);
    __syncthreads();
    for (int ch = (int)threadIdx.x; ch < C; ch += 256) {
        float wk[WV_K0];
#pragma unroll
        for (int k = 0; k < WV_K0; k++) wk[k] = w[ch * WV_K0 + k];
        const float b = bias ? bias[ch] : 0.f;
        double s = 0.0, q = 0.0;
        for (int f = 0; f < nf; f++) {
            const double y = (double)w2v_conv10(xs + f * stride, wk, b);
            s += y; q += y * y;
        }
        double *o = part + (((int64_t)wdx * n_part + p) * 2) * C;
        o[ch] = s; o[C + ch] = q;
    }
}
// ... the partials of an (item, channel) added in the order of the partition: scale = gamma rstd, shift = beta - mean scale (biased variance)
__global__ void k_w2v_wave_finish(const double *__restrict__ part, int n_part, int C, const int *__restrict__ t0 /* [W] */, int W,
                                  const float *__restrict__ gamma, const float *__restrict__ beta, float eps, float2 *__restrict__ ss /* [W][C] */)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= W * C) return;
    const int T0 = t0[i / C], n_sum = (T0 + WV_PART - 1) / WV_PART;      // the partials of the row that hold frames
    const int wdx = i / C, ch = i - wdx * C;
    double s = 0.0, q = 0.0;
    for (int p = 0; p < n_sum; p++) {
        const double *o = part + (((int64_t)wdx * n_part + p) * 2) * C;
        s += o[ch]; q += o[C + ch];
    }
    const double mean = s / (double)T0;
    double var = q / (double)T0 - mean * mean;
    if (var < 0.0) var = 0.0;
    const double scale = (double)gamma[ch] / sqrt(var + (double)eps);
    ss[i] = make_float2((float)scale, (float)((double)beta[ch] - mean * scale));
}
// Group form, pass 2: the convolution again (its pre-norm image is never stored), normalised, GELU, op_t rows [item][slot][C]
__global__ __launch_bounds__(256) void k_w2v_wave_group(const int16_t *__restrict__ pcm, const int64_t *__restrict__ win, const float *__restrict__ w,
                                                        const float *__restrict__ bias, const float2 *__restrict__ ss, int C /* % 2 == 0 */, int stride,
                                                        const int *__restrict__ t0 /* [W] */, int slot, op_t *__restrict__ out)
{
    const int T0 = t0[blockIdx.y];
    if ((int)blockIdx.x * WV_TILE >= T0) return;
    __shared__ float xs[(WV_TILE - 1) * WV_STRIDE_MAX + 16];
    const int wdx = (int)blockIdx.y;
    const int64_t base = win[3 * wdx], s0 = win[3 * wdx + 1], n = win[3 * wdx + 2];
    const int f0 = (int)blockIdx.x * WV_TILE, nf = min(WV_TILE, T0 - f0), ns = (nf - 1) * stride + WV_K0;
    for (int i = (int)threadIdx.x; i < ns; i += 256) xs[i] = w2v_sample(pcm, base, s0, n, (int64_t)f0 * stride + i);
    __syncthreads();
    for (int ch = 2 * (int)threadIdx.x; ch < C; ch += 512) {
        float wa[WV_K0], wb[WV_K0];
#pragma unroll
        for (int k = 0; k < WV_K0; k++) { wa[k] = w[ch * WV_K0 + k]; wb[k] = w[(ch + 1) * WV_K0 + k]; }
        const float ba = bias ? bias[ch] : 0.f, bb = bias ? bias[ch + 1] : 0.f;
        const float2 sa = ss[(int64_t)wdx * C + ch], sb = ss[(int64_t)wdx * C + ch + 1];
        op_t *o = out + ((int64_t)wdx * slot + f0) * C + ch;
        for (int f = 0; f < nf; f++) {
            const float ya = w2v_conv10(xs + f * stride, wa, ba), yb = w2v_conv10(xs + f * stride, wb, bb);
            opx2 v;
            v[0] = (op_t)gelu_exact(fmaf(ya, sa.x, sa.y)); v[1] = (op_t)gelu_exact(fmaf(yb, sb.x, sb.y));
            *reinterpret_cast<opx2 *>(o + (int64_t)f * C) = v;
        }
    }
}
// Layer form: convolution + bias into an LDS tile [frame][channel], then one wave per frame: LayerNorm over the channels (fp32, two-pass), GELU.
// A block behind its item's last frame leaves before the first barrier (the whole block: blockIdx decides)
__global__ __launch_bounds__(256) void k_w2v_wave_layer(const int16_t *__restrict__ pcm, const int64_t *__restrict__ win, const float *__restrict__ w,
                                                        const float *__restrict__ bias, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                        int C /* <= WV_C_MAX */, int stride, const int *__restrict__ t0 /* [W] */, int slot, float eps,
                                                        op_t *__restrict__ out)
{
    const int T0 = t0[blockIdx.y];
    if ((int)blockIdx.x * WV_LN_F >= T0) return;
    __shared__ float xs[(WV_LN_F - 1) * WV_STRIDE_MAX + 16];
    __shared__ float tile[WV_LN_F * WV_C_MAX];
    const int wdx = (int)blockIdx.y, lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int64_t base = win[3 * wdx], s0 = win[3 * wdx + 1], n = win[3 * wdx + 2];
    const int f0 = (int)blockIdx.x * WV_LN_F, nf = min(WV_LN_F, T0 - f0), ns = (nf - 1) * stride + WV_K0;
    for (int i = (int)threadIdx.x; i < ns; i += 256) xs[i] = w2v_sample(pcm, base, s0, n, (int64_t)f0 * stride + i);
    __syncthreads();
    for (int ch = (int)threadIdx.x; ch < C; ch += 256) {
        float wk[WV_K0];
#pragma unroll
        for (int k = 0; k < WV_K0; k++) wk[k] = w[ch * WV_K0 + k];
        const float b = bias ? bias[ch] : 0.f;
        for (int f = 0; f < nf; f++) tile[f * C + ch] = w2v_conv10(xs + f * stride, wk, b);
    }
    __syncthreads();
    for (int f = wv; f < nf; f += 4) {                              // (wave-uniform: the DPP reductions see whole waves)
        const float *row = tile + f * C;
        float s = 0.f;
        for (int ch = lane; ch < C; ch += 64) s += row[ch];
        const float mean = wave_dpp_sum_f32(s) / (float)C;
        float q = 0.f;
        for (int ch = lane; ch < C; ch += 64) { const float a = row[ch] - mean; q += a * a; }
        const float inv = rsqrtf(wave_dpp_sum_f32(q) / (float)C + eps);
        op_t *o = out + ((int64_t)wdx * slot + f0 + f) * C;
        for (int ch = lane; ch < C; ch += 64) o[ch] = (op_t)gelu_exact((row[ch] - mean) * inv * gamma[ch] + beta[ch]);
    }
}

// LayerNorm over the channels of 16-bit rows (one wave per row, the row in registers: C % 8 == 0, C <= LN_D_MAX), then GELU where asked: the
// layer form's convolutions 1-6 (in place: a wave reads its whole row before it writes) and the feature projection's LayerNorm.
template <bool GELU>
__global__ __launch_bounds__(256) void k_w2v_ln16(const op_t *x, const float *__restrict__ w, const float *__restrict__ b, int64_t rows, int C, float eps,
                                                  op_t *out)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = (int)threadIdx.x & 63;
    if (row >= rows) return;
    const int nc = C >> 3;
    float v[4][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int idx = lane + 64 * i;
        opx8 t = {};
        if (idx < nc) t = *reinterpret_cast<const opx8 *>(x + row * C + 8 * idx);
#pragma unroll
        for (int e = 0; e < 8; e++) v[i][e] = idx < nc ? (float)t[e] : 0.f;
        s += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
    }
    const float mean = wave_dpp_sum_f32(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (lane + 64 * i < nc) {
#pragma unroll
            for (int e = 0; e < 8; e++) { const float a = v[i][e] - mean; q += a * a; }
        }
    const float inv = rsqrtf(wave_dpp_sum_f32(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int idx = lane + 64 * i;
        if (idx < nc) {
            opx8 o;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float y = (v[i][e] - mean) * inv * w[8 * idx + e] + b[8 * idx + e];
                o[e] = (op_t)(GELU ? gelu_exact(y) : y);
            }
            *reinterpret_cast<opx8 *>(out + row * C + 8 * idx) = o;
        }
    }
}

// Positional convolution: out = x + GELU(Conv1d(d, d, 128, padding 64, groups G)(x) + bias), the last output frame of the convolution dropped, so
// frame t reads frames t - 64 .. t + 63 of its own window (zeros outside [0, T)).  One workgroup = one group's CG = d / G output columns x
// PC_MT frames of one window.  Rows t0 - 64 .. t0 + PC_MT + 63 of the group's CG input channels are rounded to op_t into LDS once; the product
// is a GEMM over K = (tap, channel) whose A fragment of tap k is the same image read k rows further down, so the staged rows serve all 128 taps.
// The weights [column][tap][channel] stream from L2 straight into the B fragments (16 bytes per lane: 8 channels of one tap, CG % 8 == 0).
// Four waves x 64 frames; v_mfma_f32_16x16x32: lane (m = lane & 15, g = lane >> 4) gives A[m][8 g ..], B[8 g ..][m] and holds D[4 g + i][m].
// LDS rows are CG + 8 elements apart: the 16 rows of a fragment read start 16 bytes x an odd multiple apart and meet no bank twice.
// Window z holds len[z] <= rows_per_win frames: the halo's zeros, the wave-uniform skip and the epilogue's t < T follow it.
template <int CG>
__global__ __launch_bounds__(256) void k_w2v_posconv(const float *__restrict__ x /* [window][rows_per_win][d] */, const op_t *__restrict__ w,
                                                     const float *__restrict__ bias, const int *__restrict__ len /* [windows] */, int rows_per_win, int d,
                                                     float *__restrict__ out)
{
    const int T = len[blockIdx.z];
    constexpr int LD = CG + 8, NB = CG / 16, TPR = CG / 4, KT = PC_TAPS * CG / 32;
    __shared__ __attribute__((aligned(16))) op_t xs[PC_ROWS * LD];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, m = lane & 15, g4 = lane >> 4;
    const int t0 = (int)blockIdx.x * PC_MT, grp = (int)blockIdx.y;
    const int64_t row0 = (int64_t)blockIdx.z * rows_per_win;
    for (int i = tid; i < PC_ROWS * TPR; i += 256) {
        const int r = i / TPR, c4 = (i - r * TPR) * 4, t = t0 - PC_TAPS / 2 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0 && t < T) v = *reinterpret_cast<const float4 *>(x + (row0 + t) * d + grp * CG + c4);
        opx4_w o; o[0] = (op_t)v.x; o[1] = (op_t)v.y; o[2] = (op_t)v.z; o[3] = (op_t)v.w;
        *reinterpret_cast<opx4_w *>(xs + r * LD + c4) = o;
    }
    __syncthreads();
    f32x4 acc[4][NB];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int nb = 0; nb < NB; nb++) acc[a][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t0 + wv * 64 < T) {                                       // (wave-uniform) a wave whose 64 frames lie behind the window's last has no product
        const op_t *wb = w + (int64_t)(grp * CG + m) * (PC_TAPS * CG) + 8 * g4;
        const op_t *xa = xs + (wv * 64 + m) * LD;
#pragma unroll 4
        for (int s = 0; s < KT; s++) {
            const int kk = s * 32 + 8 * g4, k = kk / CG, ci = kk - k * CG;
            opx8 a[4], b[NB];
#pragma unroll
            for (int nb = 0; nb < NB; nb++) b[nb] = *reinterpret_cast<const opx8 *>(wb + (int64_t)nb * 16 * (PC_TAPS * CG) + s * 32);
#pragma unroll
            for (int mb = 0; mb < 4; mb++) a[mb] = *reinterpret_cast<const opx8 *>(xa + (mb * 16 + k) * LD + ci);
#pragma unroll
            for (int mb = 0; mb < 4; mb++)
#pragma unroll
                for (int nb = 0; nb < NB; nb++) acc[mb][nb] = mfma16(a[mb], b[nb], acc[mb][nb]);
        }
    }
#pragma unroll
    for (int mb = 0; mb < 4; mb++)
#pragma unroll
        for (int nb = 0; nb < NB; nb++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int t = t0 + wv * 64 + mb * 16 + 4 * g4 + i, col = grp * CG + nb * 16 + m;
                if (t >= rows_per_win) continue;
                const int64_t idx = (row0 + t) * d + col;
                const float h = x[idx];
                out[idx] = t < T ? h + gelu_exact(acc[mb][nb][i] + bias[col]) : h;       // (a pad row: any finite value)
            }
}

// The tail: frames [cut, cut + n_keep) of every window, log-softmax in fp32 over the V real columns of the padded logits, a zero <star> column
// behind them where asked, packed at the window's place among its clip's kept frames.  One wave per frame.
__global__ __launch_bounds__(256) void k_w2v_tail(const float *__restrict__ logits /* [window][rows_per_win][Vp] */, int Vp, int V, int star,
                                                  const int64_t *__restrict__ tab /* [W][2]: first output row, frames kept */, int rows_per_win, int cut,
                                                  float *__restrict__ out, int n_cols)
{
    const int wdx = (int)blockIdx.y, lane = (int)threadIdx.x & 63;
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= tab[2 * wdx + 1]) return;
    const float *src = logits + ((int64_t)wdx * rows_per_win + cut + f) * Vp;
    float *dst = out + (tab[2 * wdx] + f) * n_cols;
    float mx = -INFINITY;
    for (int j = lane; j < V; j += 64) mx = fmaxf(mx, src[j]);
    mx = wave_xor_max(mx);
    float s = 0.f;
    for (int j = lane; j < V; j += 64) s += expf(src[j] - mx);
    const float ls = logf(wave_dpp_sum_f32(s));
    for (int j = lane; j < V; j += 64) dst[j] = (src[j] - mx) - ls;
    if (star && lane == 0) dst[V] = 0.f;
}

static int64_t w2v_frames_of(int64_t samples) { return (int64_t)((double)samples / 16000.0 * 50.0); }      // int(seconds * 50), as the host restatement rounds
static int w2v_rows_pad(int T) { return (int)div_up(T, 16) * 16; }

// Which tiled kernel computes a product: by N and K alone (launch_gemm's rule also looks at the row count, and the rows here follow the chunk).
// false, and nothing launched, for a shape the chosen kernel does not compute exactly (w2v_check's limits keep that from happening: N % 128,
// K % 64, the V columns from a multiple of 128 on)
template <int EPI>
static bool w2v_gemm(pce_ctx *c, const op_t *A, int64_t lda, int64_t a_batch, const op_t *B, int M, int N, int K, const float *bias, void *C, int64_t ldc,
                     int64_t c_batch, int batch, const float *pos = nullptr, int pos_T = 1, int v_col0 = 0, int vt_sp = AT_SP)
{
    const GemmShape s{M, N, K, lda, batch, v_col0};
    const int kind = (gemm_fits<EPI>(GK_WIDE, s) && N >= 1536) ? GK_WIDE : GK_128;
    if (!gemm_fits<EPI>(kind, s)) return false;
    launch_gemm_kernel<EPI>(c, kind, A, lda, a_batch, B, M, N, K, bias, C, ldc, c_batch, batch, pos, pos_T, v_col0, vt_sp);
    return true;
}
struct W2vGemm {                       // encoder_walk's GEMM rule for this model
    template <int EPI, class... A> static bool run(pce_ctx *c, A... a) { return w2v_gemm<EPI>(c, a...); }
};
// (pce_selftest_encoder_walk's walk under this rule, declared in pce_whisper_selftest.inc)
static bool selftest_walk_w2v(pce_ctx *c, const EncoderRun &r, const std::vector<EncoderLayerW> &layers, bool pre_ln, const WalkCapture &probe)
{
    return encoder_walk<W2vGemm>(c, r, layers, pre_ln, probe);
}

// n_win windows of len[i] <= rows_per_win frames (device table) in slots of rows_per_win rows, `frames` of them in all (the timer's work count)
static void w2v_launch_posconv(pce_ctx *c, const float *x, const op_t *w, const float *bias, const int *len, double frames, int rows_per_win, int d, int groups,
                               int n_win, float *out)
{
    const int cg = d / groups;
    const dim3 grid((unsigned)div_up(rows_per_win, PC_MT), (unsigned)groups, (unsigned)n_win), block(256);
    KernelTimer kt(c, PCE_K_W2V_POSCONV, nullptr, 2.0 * frames * d * PC_TAPS * cg);
    switch (cg) {
    case 16: hipLaunchKernelGGL(k_w2v_posconv<16>, grid, block, 0, c->stream, x, w, bias, len, rows_per_win, d, out); break;
    case 32: hipLaunchKernelGGL(k_w2v_posconv<32>, grid, block, 0, c->stream, x, w, bias, len, rows_per_win, d, out); break;
    case 48: hipLaunchKernelGGL(k_w2v_posconv<48>, grid, block, 0, c->stream, x, w, bias, len, rows_per_win, d, out); break;
    default: hipLaunchKernelGGL(k_w2v_posconv<64>, grid, block, 0, c->stream, x, w, bias, len, rows_per_win, d, out); break;
    }
}
static bool w2v_posconv_fits(int d, int groups)
{
    if (groups <= 0 || d <= 0 || d % groups) return false;
    const int cg = d / groups;
    return cg == 16 || cg == 32 || cg == 48 || cg == 64;
}

// the waveform layer of n_win windows of pcm: group form (feat_norm 0: statistics, finish, recompute) or layer form (1).  Window i holds
// d_t0[i] <= slot frames (device table) in a slot of `slot` rows, `frames` of them in all (the timer's work count)
static int w2v_launch_wave(pce_ctx *c, int feat_norm, const int16_t *pcm, const int64_t *d_win, const int *d_t0, double frames, int n_win, const float *w,
                           const float *bias, const float *gamma, const float *beta, int C, int stride, int slot, DevBuf &part, DevBuf &ss, op_t *out)
{
    KernelTimer kt(c, PCE_K_W2V_WAVE, nullptr, 2.0 * frames * C * WV_K0 * (feat_norm == 0 ? 2 : 1));
    if (feat_norm == 0) {
        const int n_part = (int)div_up(slot, WV_PART);
        PCE_HIP(c, part.reserve(sizeof(double) * (size_t)n_win * n_part * 2 * C));
        PCE_HIP(c, ss.reserve(sizeof(float2) * (size_t)n_win * C));
        const dim3 g_stats((unsigned)n_part, (unsigned)n_win), g_fin((unsigned)div_up((int64_t)n_win * C, 256)), g_group((unsigned)div_up(slot, WV_TILE), (unsigned)n_win);
        hipLaunchKernelGGL(k_w2v_wave_stats, g_stats, dim3(256), 0, c->stream, pcm, d_win, w, bias, C, stride, d_t0, n_part, part.as<double>());
        hipLaunchKernelGGL(k_w2v_wave_finish, g_fin, dim3(256), 0, c->stream, part.as<double>(), n_part, C, d_t0, n_win, gamma, beta, 1e-5f, ss.as<float2>());
        hipLaunchKernelGGL(k_w2v_wave_group, g_group, dim3(256), 0, c->stream, pcm, d_win, w, bias, ss.as<float2>(), C, stride, d_t0, slot, out);
    } else {
        const dim3 grid((unsigned)div_up(slot, WV_LN_F), (unsigned)n_win);
        hipLaunchKernelGGL(k_w2v_wave_layer, grid, dim3(256), 0, c->stream, pcm, d_win, w, bias, gamma, beta, C, stride, d_t0, slot, 1e-5f, out);
    }
    return PCE_OK;
}
static void w2v_launch_ln16(pce_ctx *c, bool gelu, const op_t *x, const float *w, const float *b, int64_t rows, int C, float eps, op_t *out)
{
    const dim3 grid((unsigned)div_up(rows, 4)), block(256);
    if (gelu) hipLaunchKernelGGL(k_w2v_ln16<true>, grid, block, 0, c->stream, x, w, b, rows, C, eps, out);
    else hipLaunchKernelGGL(k_w2v_ln16<false>, grid, block, 0, c->stream, x, w, b, rows, C, eps, out);
}

// floats of the weight blob (w2v_weights.tensor_order)
static int64_t w2v_blob_floats(const pce_w2v_dims &m)
{
    const bool layer = m.feat_norm == 1;
    int64_t n = 0;
    for (int i = 0; i < m.n_conv; i++) {
        const int64_t cin = i ? m.conv_dim[i - 1] : 1, co = m.conv_dim[i];
        n += co * cin * m.conv_kernel[i] + (m.conv_bias ? co : 0) + ((layer || i == 0) ? 2 * co : 0);
    }
    const int64_t d = m.n_state, c6 = m.conv_dim[m.n_conv - 1], I = m.n_inter;
    n += 2 * c6 + d * c6 + d;                                             // feature projection: LayerNorm, projection
    n += d * (d / m.pos_groups) * m.pos_taps + d + 2 * d;                 // positional convolution (folded), encoder LayerNorm
    n += (int64_t)m.n_layer * (4 * (d * d + d) + 2 * d + (I * d + I) + (d * I + d) + 2 * d);
    return n + (int64_t)m.n_vocab * d + m.n_vocab;
}

// The loader's conditions, host arithmetic only (pce_w2v_check hands them out without a context): status and its message
static int w2v_refuse(char *msg, size_t cap, int code, const char *fmt, ...) __attribute__((format(printf, 4, 5)));
static int w2v_refuse(char *msg, size_t cap, int code, const char *fmt, ...)
{
    if (msg && cap) { va_list ap; va_start(ap, fmt); vsnprintf(msg, cap, fmt, ap); va_end(ap); }
    return code;
}
static int w2v_check(const pce_w2v_dims &m, int64_t n_floats, char *msg, size_t cap)
{
    const int d = m.n_state, I = m.n_inter, L = m.n_layer, V = m.n_vocab;
    if (m.n_conv != 7) return w2v_refuse(msg, cap, PCE_E_LIMIT, "wav2vec2 with %d feature-encoder layers (the run path holds 7)", m.n_conv);
    if (m.feat_norm != 0 && m.feat_norm != 1) return w2v_refuse(msg, cap, PCE_E_INVALID, "feat_norm %d (0 = group, 1 = layer)", m.feat_norm);
    if (m.conv_kernel[0] != WV_K0 || m.conv_stride[0] < 1 || m.conv_stride[0] > WV_STRIDE_MAX)
        return w2v_refuse(msg, cap, PCE_E_LIMIT, "waveform layer with %d taps at stride %d (the kernel holds %d taps, stride <= %d)", m.conv_kernel[0], m.conv_stride[0], WV_K0,
                        WV_STRIDE_MAX);
    for (int i = 0; i < 7; i++) {
        const int co = m.conv_dim[i];
        if (co <= 0 || co % 64 || co > WV_C_MAX || (i && co % 128) || m.conv_kernel[i] < 1 || m.conv_stride[i] < 1)
            return w2v_refuse(msg, cap, PCE_E_LIMIT, "conv layer %d: %d channels, %d taps, stride %d (channels %% 64 == 0 and <= %d, %% 128 == 0 behind the waveform layer)", i,
                            co, m.conv_kernel[i], m.conv_stride[i], WV_C_MAX);
        if (i && ((int64_t)m.conv_kernel[i] * m.conv_dim[i - 1]) % 64)
            return w2v_refuse(msg, cap, PCE_E_LIMIT, "conv layer %d: K = %d taps x %d channels is no multiple of 64 (the GEMM's K step)", i, m.conv_kernel[i], m.conv_dim[i - 1]);
    }
    if (d <= 0 || d % 128 || m.n_head * 64 != d || L <= 0 || V <= 0)
        return w2v_refuse(msg, cap, PCE_E_LIMIT, "unsupported wav2vec2 dims (need n_state %% 128 == 0, head size 64, n_layer >= 1, n_vocab >= 1)");
    if (d > LN_D_MAX) return w2v_refuse(msg, cap, PCE_E_LIMIT, "wav2vec2 with n_state %d: the LayerNorm kernels hold at most %d", d, LN_D_MAX);
    if (I <= 0 || I % 128) return w2v_refuse(msg, cap, PCE_E_LIMIT, "n_inter %d is no multiple of 128 (the GEMM's column tile)", I);
    if (m.pos_taps != PC_TAPS) return w2v_refuse(msg, cap, PCE_E_LIMIT, "positional convolution with %d taps (the kernel holds %d)", m.pos_taps, PC_TAPS);
    if (!w2v_posconv_fits(d, m.pos_groups))
        return w2v_refuse(msg, cap, PCE_E_LIMIT, "positional convolution: n_state %d in %d groups (need 16, 32, 48 or 64 columns per group)", d, m.pos_groups);
    if (!(m.ln_eps > 0.f)) return w2v_refuse(msg, cap, PCE_E_INVALID, "ln_eps must be positive");
    const int64_t expect = w2v_blob_floats(m);
    if (n_floats != expect) return w2v_refuse(msg, cap, PCE_E_INVALID, "wav2vec2 weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)expect);
    return PCE_OK;
}

// A run as the host describes it: items (the windows of pce_w2v_run, the segments of pce_w2v_run_segments) in chunks that go through one set
// of launches each, and the tables those launches read.  An item's slot in its chunk is Tl[i] rows behind convolution i (T_pad behind the
// last, whose frames are Tl[6]) and T_pad rows from there on; the item itself holds t0[] waveform frames and len[] frames.
struct W2vChunk {
    int64_t first; int n_win;           // items [first, first + n_win) of win and tail
    int64_t tab;                        // the chunk's first entry of t0, row0 and len
    int Tl[7], T_pad, vt_sp;            // the slot; columns of a row of V^T
    int tail_frames;                    // frames an item keeps, at most (the tail's grid)
    double wave_frames, frames, attn_flops;      // the timers' work counts: waveform frames, frames and attention flops of the chunk's items
};
struct W2vRun {
    std::vector<W2vChunk> chunks;
    std::vector<int64_t> win;           // [item][3]: first sample of the clip, the item's first sample relative to it, samples it may read
    std::vector<int64_t> tail;          // [item][2]: first row of b.em, frames kept
    std::vector<int> t0, row0, len;     // waveform frames; first row of the slot in its chunk; frames (attention, positional convolution)
    int64_t rows_total = 0;             // rows of b.em
    int cut = 0, star = 0, n_cols = 0;  // frames dropped in front of every item; the <star> column; columns of b.em
};
static W2vChunk w2v_chunk(int64_t first, int n_win, int64_t tab, const int *Tl)
{
    W2vChunk k{};
    k.first = first; k.n_win = n_win; k.tab = tab;
    std::copy(Tl, Tl + 7, k.Tl);
    k.T_pad = w2v_rows_pad(Tl[6]); k.vt_sp = (int)div_up(Tl[6], 64) * 64;
    return k;
}

// One chunk through the whole model, from the resident PCM to its rows of b.em (the run's tables are on the device: w2v_run_chunks)
static int w2v_forward_chunk(pce_ctx *c, WhisperState::W2v &b, const W2vRun &run, const W2vChunk &k, bool &fit)
{
    const pce_w2v_dims &m = b.dims;
    const int d = m.n_state, H = m.n_head, I = m.n_inter, V = m.n_vocab, Vp = b.Vp, C6 = m.conv_dim[6];
    const int Wc = k.n_win, T_pad = k.T_pad, M = Wc * T_pad;
    const int *Tl = k.Tl;
    const int *t0 = b.t0tab.as<int>() + k.tab, *row0 = b.atab.as<int>() + k.tab, *len = row0 + run.row0.size();
    const op_t *Wb = b.w16.as<op_t>();
    const float *Wf = b.w32.as<float>();
    const float eps = m.ln_eps;
    {   // the feature encoder
        const WhisperState::W2v::Conv &c0 = b.conv[0];
        PCE_TRY(w2v_launch_wave(c, m.feat_norm, c->d_pcm, b.wintab.as<int64_t>() + 3 * k.first, t0, k.wave_frames, Wc, Wf + c0.w, c0.has_b ? Wf + c0.b : nullptr,
                                Wf + c0.g, Wf + c0.beta, m.conv_dim[0], m.conv_stride[0], Tl[0], b.part, b.ss, b.img[0].as<op_t>()));
        for (int i = 1; i < 7; i++) {
            const WhisperState::W2v::Conv &cv = b.conv[i];
            const int ci = m.conv_dim[i - 1], co = m.conv_dim[i];
            const op_t *src = b.img[(i - 1) & 1].as<op_t>();
            op_t *dst = b.img[i & 1].as<op_t>();
            const int64_t rows_out = i == 6 ? T_pad : Tl[i];
            const float *bias = cv.has_b ? Wf + cv.b : nullptr;
            if (cv.has_ln) {
                fit &= w2v_gemm<EPI_BF16>(c, src, (int64_t)m.conv_stride[i] * ci, (int64_t)Tl[i - 1] * ci, Wb + cv.w, Tl[i], co, m.conv_kernel[i] * ci, bias, dst, co,
                                   rows_out * co, Wc);
                w2v_launch_ln16(c, true, dst, Wf + cv.g, Wf + cv.beta, (int64_t)Wc * rows_out, co, 1e-5f, dst);
            } else {
                fit &= w2v_gemm<EPI_GELU_BF16>(c, src, (int64_t)m.conv_stride[i] * ci, (int64_t)Tl[i - 1] * ci, Wb + cv.w, Tl[i], co, m.conv_kernel[i] * ci, bias, dst,
                                        co, rows_out * co, Wc);
            }
        }
    }
    // feature projection, positional convolution
    w2v_launch_ln16(c, false, b.img[0].as<op_t>(), Wf + b.fp_ln_w, Wf + b.fp_ln_b, M, C6, eps, b.fpln.as<op_t>());
    fit &= w2v_gemm<EPI_F32>(c, b.fpln.as<op_t>(), C6, 0, Wb + b.proj_w, M, d, C6, Wf + b.proj_b, b.h0.as<float>(), d, 0, 1);
    w2v_launch_posconv(c, b.h0.as<float>(), Wb + b.pos_w, Wf + b.pos_b, len, k.frames, T_pad, d, m.pos_groups, Wc, b.h.as<float>());
    const bool pre = m.stable_ln != 0;
    const EncoderRun r{M, d, H, I, Wc, T_pad, k.vt_sp, row0, len, eps, k.attn_flops, false, b.h.as<float>(), b.ln.as<op_t>(), b.qk.as<op_t>(),
                       b.vt.as<op_t>(), b.attn.as<op_t>(), b.hidden.as<op_t>(), Wb, Wf};
    // the encoder LayerNorm: in front of a post-LN stack (in place on the fp32 stream, and its op_t copy), behind a pre-LN one
    if (!pre) launch_layernorm<op_t>(c, b.h.as<float>(), Wf + b.enc_ln_w, Wf + b.enc_ln_b, M, d, b.ln.as<op_t>(), eps, b.h.as<float>());
    fit &= encoder_walk<W2vGemm>(c, r, b.layers, pre);
    if (pre) launch_layernorm<op_t>(c, b.h.as<float>(), Wf + b.enc_ln_w, Wf + b.enc_ln_b, M, d, b.ln.as<op_t>(), eps);
    fit &= w2v_gemm<EPI_F32>(c, b.ln.as<op_t>(), d, 0, Wb + b.lm_w, M, Vp, d, Wf + b.lm_b, b.logits.as<float>(), Vp, 0, 1);
    {
        KernelTimer kt(c, PCE_K_W2V_TAIL);
        hipLaunchKernelGGL(k_w2v_tail, dim3((unsigned)div_up(k.tail_frames, 4), (unsigned)Wc), dim3(256), 0, c->stream, b.logits.as<float>(), Vp, V, run.star,
                           b.tailtab.as<int64_t>() + 2 * k.first, T_pad, run.cut, b.em.as<float>(), run.n_cols);
    }
    PCE_HIP(c, hipGetLastError());
    if (!fit) return pce_fail(c, PCE_E_LIMIT, "a product of this model has a shape the tiled GEMM kernels do not compute (N %% 128, K %% 64)");
    return PCE_OK;
}
// bytes of one window's activation images in a chunk whose slots hold Tl[] rows (the two ping-pong convolution images, the encoder's buffers)
static int64_t w2v_slot_bytes(const pce_w2v_dims &m, int Vp, const int *Tl, int64_t *img_e /* [2]: elements of the two convolution images */)
{
    const int d = m.n_state, I = m.n_inter, C6 = m.conv_dim[6], T_pad = w2v_rows_pad(Tl[6]), vt_sp = (int)div_up(Tl[6], 64) * 64;
    img_e[0] = img_e[1] = 0;
    for (int i = 0; i < 7; i++) img_e[i & 1] = std::max<int64_t>(img_e[i & 1], (int64_t)(i == 6 ? T_pad : Tl[i]) * m.conv_dim[i]);
    return 2 * (img_e[0] + img_e[1]) + (int64_t)T_pad * (2LL * C6 + 8LL * d + 2LL * d + 4LL * d + 2LL * d + 2LL * I + 4LL * Vp) + 2LL * d * vt_sp +
           (m.feat_norm == 0 ? 16LL * div_up(Tl[0], WV_PART) * m.conv_dim[0] : 0);
}

// The run: buffers for the largest chunk, the tables, the clears, the chunks.  A chunk's launches cover n_win slots of its own rows, every item's
// own frame counts in the tables of the waveform layer, the positional convolution, the attention and the tail.
//
// Rows behind an item's own frames, and why nothing that is not finite sits in them although the slot stride changes from chunk to chunk.
// A real row reads pad rows of its own slot in one place only: the attention multiplies the V^T columns of masked keys by probabilities that
// are exactly zero, so those columns must be finite; everything else a real row reads is a real row of its slot (a convolution row t < Tl[i]
// reads rows < Tl[i - 1], the positional convolution takes frames >= len as zeros, GEMM and LayerNorm rows are independent).  The pad rows are
// finite by induction over the launches.  Every buffer but three is written in all rows of all slots of a chunk before the
// chunk reads it (img[1], fpln, h0, h, ln, qk, hidden, logits: GEMM, LayerNorm and positional-convolution launches cover M = slots x rows), so
// what an earlier chunk or call left there under another stride is never read.  The three that a chunk writes in part are img[0] (the waveform
// layer writes t < t0 of a slot of Tl[0] rows; the last convolution Tl[6] of T_pad rows), attn (the attention writes queries < len) and vt (the
// V epilogue writes keys < T_pad of vt_sp columns).  Their other elements hold what an earlier chunk stored there under its own stride, and
// that is always a value one of these kernels stored for some row -- a GELU or LayerNorm output, an attention output, a V projection, computed
// from finite inputs -- or the zero of the clear below: the three are cleared over the largest extent any chunk of this call uses before the
// first launch, so no element is read that this call or the clear did not write (a buffer that grew holds fresh memory).  Stale rows are
// therefore finite under any stride, and a finite pad row gives finite pad rows downstream (no kernel divides by a row's own values but the
// LayerNorms, whose eps > 0 keeps a constant row finite).
static int w2v_run_chunks(pce_ctx *c, WhisperState::W2v &b, const W2vRun &run)
{
    const pce_w2v_dims &m = b.dims;
    const int d = m.n_state, I = m.n_inter, Vp = b.Vp, C6 = m.conv_dim[6];
    int64_t img0 = 0, img1 = 0, M_max = 0, vt_max = 0;
    for (const W2vChunk &k : run.chunks) {
        int64_t e[2];
        w2v_slot_bytes(m, Vp, k.Tl, e);
        img0 = std::max(img0, k.n_win * e[0]); img1 = std::max(img1, k.n_win * e[1]);
        M_max = std::max(M_max, (int64_t)k.n_win * k.T_pad); vt_max = std::max(vt_max, (int64_t)k.n_win * d * k.vt_sp);
    }
    PCE_HIP(c, b.img[1].reserve(sizeof(op_t) * (size_t)img1 + 4096));
    PCE_HIP(c, b.fpln.reserve(sizeof(op_t) * (size_t)M_max * C6 + 4096));
    PCE_HIP(c, b.h0.reserve(sizeof(float) * (size_t)M_max * d));
    PCE_HIP(c, b.h.reserve(sizeof(float) * (size_t)M_max * d));
    PCE_HIP(c, b.ln.reserve(sizeof(op_t) * (size_t)M_max * d + 4096));
    PCE_HIP(c, b.qk.reserve(sizeof(op_t) * (size_t)M_max * 2 * d + 4096));
    PCE_HIP(c, b.hidden.reserve(sizeof(op_t) * (size_t)M_max * I + 4096));
    PCE_HIP(c, b.logits.reserve(sizeof(float) * (size_t)M_max * Vp));
    PCE_HIP(c, b.em.reserve(sizeof(float) * (size_t)run.rows_total * run.n_cols + 256));
    std::vector<int> at(run.row0);                              // the attention's two tables in one buffer: every row0, then every len
    at.insert(at.end(), run.len.begin(), run.len.end());
    PCE_UPLOAD(c, b.wintab, run.win);
    PCE_UPLOAD(c, b.tailtab, run.tail);
    PCE_UPLOAD(c, b.t0tab, run.t0);
    PCE_UPLOAD(c, b.atab, at);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    // what the argument above needs cleared: the three buffers a chunk writes in part, over the largest extent any chunk uses
    PCE_ZERO(op_t, c, b.img[0], (size_t)img0 + 2048);
    PCE_ZERO(op_t, c, b.attn, (size_t)M_max * d + 2048);
    PCE_ZERO(op_t, c, b.vt, (size_t)vt_max + 64);
    KernelTimer timer(c, PCE_K_W2V);
    bool fit = true;                                             // every product's shape fits its kernel (w2v_gemm)
    for (const W2vChunk &k : run.chunks) PCE_TRY(w2v_forward_chunk(c, b, run, k, fit));
    return PCE_OK;
}

// the waveform layer's selftests: items tab[i] of t0[i] frames of pcm through the run's launches into out [item][slot][C], slot = the longest
// item's frames; rows behind an item's frames are left as the zeros out is cleared to
static int w2v_selftest_wave(pce_ctx *c, const int16_t *pcm, int64_t n_samples, const std::vector<int64_t> &tab, const std::vector<int> &t0, int feat_norm, int C,
                             int stride, const float *w, const float *bias, const float *gamma, const float *beta, uint16_t *out)
{
    const int n_win = (int)t0.size(), slot = *std::max_element(t0.begin(), t0.end());
    double frames = 0.0;
    for (const int t : t0) frames += (double)t;
    DevBuf dp, dt, d0, dw, db, dg, dbe, part, ss, dout;
    const size_t n_out = (size_t)n_win * (size_t)slot * C;
    PCE_UPLOAD(c, dp, pcm, (size_t)n_samples); PCE_UPLOAD(c, dt, tab); PCE_UPLOAD(c, d0, t0); PCE_UPLOAD(c, dw, w, (size_t)C * WV_K0);
    if (bias) PCE_UPLOAD(c, db, bias, (size_t)C);
    PCE_UPLOAD(c, dg, gamma, (size_t)C); PCE_UPLOAD(c, dbe, beta, (size_t)C);
    PCE_ZERO(op_t, c, dout, n_out);
    PCE_TRY(w2v_launch_wave(c, feat_norm, dp.as<int16_t>(), dt.as<int64_t>(), d0.as<int>(), frames, n_win, dw.as<float>(), bias ? db.as<float>() : nullptr,
                            dg.as<float>(), dbe.as<float>(), C, stride, slot, part, ss, dout.as<op_t>()));
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, out, dout.p, n_out);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

} // namespace

namespace PCE_BUILD_NS {

int pce_w2v_check(const pce_w2v_dims *dims, int64_t n_floats, char *msg, size_t cap)
{
    if (msg && cap) msg[0] = 0;
    return dims ? w2v_check(*dims, n_floats, msg, cap) : PCE_E_INVALID;
}

int pce_w2v_load(pce_ctx *c, const pce_w2v_dims *dims, const float *weights, int64_t n_floats)
{
    if (!c || !dims || !weights) return PCE_E_INVALID;
    const pce_w2v_dims &m = *dims;
    const int d = m.n_state, I = m.n_inter, L = m.n_layer, V = m.n_vocab;
    {
        char msg[320];
        const int rc = w2v_check(m, n_floats, msg, sizeof msg);
        if (rc) return pce_fail(c, rc, "%s", msg);
    }
    PCE_HIP(c, hipSetDevice(c->device));
    WhisperState::W2v &b = ws_of(c)->w2v;
    b.dims = m; b.loaded = false; b.n_clips = -1; b.layers.assign((size_t)L, {});
    WeightPack pk;
    const bool layer = m.feat_norm == 1;
    const float *p = weights;
    for (int i = 0; i < 7; i++) {
        const size_t cin = i ? (size_t)m.conv_dim[i - 1] : 1, co = (size_t)m.conv_dim[i], nw = co * cin * (size_t)m.conv_kernel[i];
        WhisperState::W2v::Conv &cv = b.conv[i];
        cv.w = i ? pk.mat(p, nw) : pk.vec(p, nw);                                  // the waveform layer's taps stay fp32
        cv.has_b = m.conv_bias != 0; cv.has_ln = layer || i == 0;
        if (cv.has_b) cv.b = pk.vec(p, co);
        if (cv.has_ln) { cv.g = pk.vec(p, co); cv.beta = pk.vec(p, co); }
    }
    const size_t c6 = (size_t)m.conv_dim[6], cg = (size_t)(d / m.pos_groups);
    b.fp_ln_w = pk.vec(p, c6); b.fp_ln_b = pk.vec(p, c6);
    b.proj_w = pk.mat(p, (size_t)d * c6); b.proj_b = pk.vec(p, (size_t)d);
    b.pos_w = pk.mat(p, (size_t)d * cg * PC_TAPS); b.pos_b = pk.vec(p, (size_t)d);
    b.enc_ln_w = pk.vec(p, (size_t)d); b.enc_ln_b = pk.vec(p, (size_t)d);
    for (EncoderLayerW &ly : b.layers) ly = pack_encoder_layer(pk, p, (size_t)d, (size_t)I, false, true);
    {   // lm_head [n_vocab][d] padded with zero rows to whole 128-column GEMM tiles
        b.Vp = (int)div_up(V, 128) * 128;
        std::vector<float> lw((size_t)b.Vp * d, 0.f), lb((size_t)b.Vp, 0.f);
        memcpy(lw.data(), p, sizeof(float) * (size_t)V * d); p += (size_t)V * d;
        memcpy(lb.data(), p, sizeof(float) * (size_t)V); p += V;
        b.lm_w = pk.mat_at(lw.data(), lw.size()); b.lm_b = pk.vec_at(lb.data(), lb.size());
    }
    DevBuf tmp;
    PCE_TRY(upload_weights(c, pk, tmp, b.w16, b.w32));
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    b.loaded = true;
    return PCE_OK;
}

int pce_w2v_run(pce_ctx *c, const pce_w2v_plan *plan)
{
    if (!c || !plan) return PCE_E_INVALID;
    WhisperState::W2v &b = ws_of(c)->w2v;
    if (!b.loaded) return pce_fail(c, PCE_E_STATE, "pce_w2v_run before pce_w2v_load");
    if (!c->d_pcm) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    if (c->rate != 16000) return pce_fail(c, PCE_E_INVALID, "wav2vec2 runs at 16000 Hz: the resident batch is at %d Hz (resample it first)", c->rate);
    const pce_w2v_dims &m = b.dims;
    const int64_t window = plan->window_samples, context = plan->context_samples;
    if (window < 1 || context < 0 || plan->windows_per_chunk < 0 || window + 2 * context > ((int64_t)1 << 26))
        return pce_fail(c, PCE_E_INVALID, "bad wav2vec2 plan (window_samples >= 1, context_samples >= 0, window + 2 context <= 2^26, windows_per_chunk >= 0)");
    int Tl[7];
    {
        int64_t t = window + 2 * context;
        for (int i = 0; i < 7; i++) { t = t >= m.conv_kernel[i] ? (t - m.conv_kernel[i]) / m.conv_stride[i] + 1 : 0; Tl[i] = (int)t; }
    }
    const int T = Tl[6], wf = (int)w2v_frames_of(window), cut = (int)w2v_frames_of(context);
    // frames [cut, T - cut + 1) of a window's T are kept (the slice ends at T at the latest)
    if (T < 1 || wf < 1 || std::min(T - cut + 1, T) - cut != wf)
        return pce_fail(c, PCE_E_INVALID, "the model gives %d frames per window of %lld + 2 x %lld samples, %d of them kept behind a cut of %d: %d expected (20 ms stride)", T,
                        (long long)window, (long long)context, std::min(T - cut + 1, T) - cut, cut, wf);
    PCE_HIP(c, hipSetDevice(c->device));
    b.n_clips = -1; b.seg_plan[0] = -1;
    const int n = c->n_clips, d = m.n_state, I = m.n_inter, V = m.n_vocab, Vp = b.Vp;
    const int T_pad = w2v_rows_pad(T), vt_sp = (int)div_up(T, 64) * 64, n_cols = V + (plan->star ? 1 : 0);
    // the attention's buffer resources and the transposed-V epilogue form 32-bit byte offsets inside one window
    if (((int64_t)T * 2 * d + 64) * 2 >= ((int64_t)1 << 31) || (int64_t)64 * vt_sp * 2 >= ((int64_t)1 << 31))
        return pce_fail(c, PCE_E_LIMIT, "%d frames per window: the attention kernel's 32-bit offsets do not reach that far", T);
    // the plan: every clip's windows, the rows its kept frames take
    W2vRun run;
    run.cut = cut; run.star = plan->star ? 1 : 0; run.n_cols = n_cols;
    b.row_start.assign((size_t)n, 0); b.n_frames.assign((size_t)n, 0);
    int64_t &rows_total = run.rows_total;
    for (int q = 0; q < n; q++) {
        const int64_t len = c->clip_off[(size_t)q + 1] - c->clip_off[(size_t)q];
        int64_t n_win, keep;
        pce_w2v_window_plan(len, (int32_t)window, (int32_t)context, &n_win, &keep);
        b.row_start[(size_t)q] = rows_total; b.n_frames[(size_t)q] = (int32_t)keep;
        for (int64_t j = 0; j < n_win; j++) {
            run.win.push_back(c->clip_off[(size_t)q]); run.win.push_back(j * window - context); run.win.push_back(len);
            run.tail.push_back(rows_total + j * wf); run.tail.push_back(std::min<int64_t>(wf, keep - j * wf));
        }
        rows_total += keep;
        if (rows_total > INT32_MAX) return pce_fail(c, PCE_E_LIMIT, "more than 2^31 emission frames in one batch");
    }
    const int64_t W = (int64_t)(run.win.size() / 3);
    b.n_cols = n_cols;
    if (W == 0) { b.n_clips = 0; return PCE_OK; }
    // chunk size: the images of one window
    int64_t img_e[2];
    const int64_t per_window = w2v_slot_bytes(m, Vp, Tl, img_e);
    int64_t wpc = plan->windows_per_chunk > 0 ? plan->windows_per_chunk : std::max<int64_t>(1, PCE_W2V_IMAGE_BUDGET / per_window);
    wpc = std::min<int64_t>(std::min<int64_t>(wpc, W), 4096);
    while (wpc > 1 && wpc * T_pad * (int64_t)std::max(std::max(3 * d, I), Vp) >= ((int64_t)1 << 31)) wpc--;      // (the launchers count rows in int)
    // equal chunks of equal windows share one range of t0, row0 and len: the largest chunk's, of which a shorter last chunk reads the front
    for (int64_t i = 0; i < wpc; i++) { run.t0.push_back(Tl[0]); run.row0.push_back((int)(i * T_pad)); run.len.push_back(T); }
    for (int64_t w0 = 0; w0 < W; w0 += wpc) {
        W2vChunk k = w2v_chunk(w0, (int)std::min<int64_t>(wpc, W - w0), 0, Tl);
        k.tail_frames = wf;
        k.wave_frames = (double)k.n_win * Tl[0]; k.frames = (double)k.n_win * T; k.attn_flops = 4.0 * k.n_win * (double)T * T * d;
        run.chunks.push_back(k);
    }
    PCE_TRY(w2v_run_chunks(c, b, run));
    b.n_clips = n;
    return PCE_OK;
}

// whisperX's emissions: the model on every segment alone (Aligners/ctc_emissions.segment_emissions), in chunks of segments of similar length
// (pce_w2v_seg_plan.h): slots of the rows of a chunk's longest segment at every layer, every segment's own frame counts in the tables, cut = 0.
int pce_w2v_run_segments(pce_ctx *c, const pce_w2v_segment *segs, int32_t n_seg, const pce_w2v_seg_plan *plan)
{
    if (!c || !plan || n_seg < 0 || (n_seg && !segs)) return PCE_E_INVALID;
    WhisperState::W2v &b = ws_of(c)->w2v;
    if (!b.loaded) return pce_fail(c, PCE_E_STATE, "pce_w2v_run_segments before pce_w2v_load");
    if (!c->d_pcm) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    if (c->rate != 16000) return pce_fail(c, PCE_E_INVALID, "wav2vec2 runs at 16000 Hz: the resident batch is at %d Hz (resample it first)", c->rate);
    if (plan->min_samples < 0 || plan->segments_per_chunk < 0) return pce_fail(c, PCE_E_INVALID, "bad segment plan (min_samples >= 0, segments_per_chunk >= 0)");
    const pce_w2v_dims &m = b.dims;
    const int d = m.n_state, I = m.n_inter, V = m.n_vocab, Vp = b.Vp, n_cols = V + (plan->star ? 1 : 0);
    const auto layer_frames = [&](int64_t samples, int *Tl) {
        int64_t t[7];
        w2v_seg_layer_frames(m.conv_kernel, m.conv_stride, 7, samples, t);
        for (int i = 0; i < 7; i++) Tl[i] = (int)t[i];
    };
    std::vector<int64_t> samples((size_t)n_seg);
    int64_t longest = 0;
    for (int j = 0; j < n_seg; j++) {
        const pce_w2v_segment &sg = segs[j];
        if (sg.clip < 0 || sg.clip >= c->n_clips) return pce_fail(c, PCE_E_INVALID, "segment %d: clip %d out of range", j, sg.clip);
        const int64_t len = c->clip_off[(size_t)sg.clip + 1] - c->clip_off[(size_t)sg.clip];
        if (sg.begin < 0 || sg.begin > sg.end || sg.end > len)
            return pce_fail(c, PCE_E_INVALID, "segment %d: samples [%lld, %lld) of a clip of %lld (need 0 <= begin <= end <= length)", j, (long long)sg.begin,
                            (long long)sg.end, (long long)len);
        samples[(size_t)j] = std::max<int64_t>(sg.end - sg.begin, plan->min_samples);
        longest = std::max(longest, samples[(size_t)j]);
    }
    if (longest > ((int64_t)1 << 26)) return pce_fail(c, PCE_E_LIMIT, "a segment of %lld samples (at most 2^26)", (long long)longest);
    {   // the attention's buffer resources and the transposed-V epilogue form 32-bit byte offsets inside one slot
        int Tl[7];
        layer_frames(longest, Tl);
        const int64_t T = Tl[6], vt_sp = div_up(T, 64) * 64;
        if ((T * 2 * d + 64) * 2 >= ((int64_t)1 << 31) || 64 * vt_sp * 2 >= ((int64_t)1 << 31))
            return pce_fail(c, PCE_E_LIMIT, "%lld frames in one segment: the attention kernel's 32-bit offsets do not reach that far", (long long)T);
    }
    PCE_HIP(c, hipSetDevice(c->device));
    b.n_clips = -1; b.seg_plan[0] = -1;
    b.row_start.assign((size_t)n_seg, 0); b.n_frames.assign((size_t)n_seg, 0);
    int64_t rows_total = 0;
    std::vector<int> t0_of((size_t)n_seg);
    for (int j = 0; j < n_seg; j++) {
        int Tl[7];
        layer_frames(samples[(size_t)j], Tl);
        if (Tl[6] < 1) return pce_fail(c, PCE_E_INVALID, "segment %d: the model gives no frame for %lld samples", j, (long long)samples[(size_t)j]);
        t0_of[(size_t)j] = Tl[0];
        b.row_start[(size_t)j] = rows_total; b.n_frames[(size_t)j] = Tl[6];
        rows_total += Tl[6];
        if (rows_total > INT32_MAX) return pce_fail(c, PCE_E_LIMIT, "more than 2^31 emission frames in one batch");
    }
    b.n_cols = n_cols;
    if (n_seg == 0) { b.n_clips = 0; b.seg_plan[0] = b.seg_plan[1] = b.seg_plan[2] = 0; return PCE_OK; }
    const int64_t row_limit = (((int64_t)1 << 31) - 1) / std::max(std::max(3 * d, I), Vp);          // (the launchers count rows in int)
    const W2vSegPlan sp = w2v_seg_plan(
        samples, plan->segments_per_chunk, PCE_W2V_IMAGE_BUDGET, row_limit, [&](int64_t s) { int Tl[7]; layer_frames(s, Tl); return (int64_t)Tl[6]; },
        [&](int64_t s) { int Tl[7]; int64_t e[2]; layer_frames(s, Tl); return w2v_slot_bytes(m, Vp, Tl, e); });
    // the run, in the plan's order: a chunk's slot is its first (longest) segment's rows at every layer
    W2vRun run;
    run.rows_total = rows_total; run.star = plan->star ? 1 : 0; run.n_cols = n_cols;
    for (const W2vSegChunk &ch : sp.chunks) {
        int Tl[7];
        layer_frames(ch.samples, Tl);
        W2vChunk k = w2v_chunk((int64_t)ch.first, (int)ch.count, (int64_t)ch.first, Tl);
        k.tail_frames = Tl[6];
        for (size_t i = 0; i < ch.count; i++) {
            const int j = sp.order[ch.first + i], nf = b.n_frames[(size_t)j];
            const pce_w2v_segment &sg = segs[j];
            // the waveform layer reads samples [0, end - begin) behind the segment's first and supplies the zeros up to min_samples itself
            run.win.push_back(c->clip_off[(size_t)sg.clip] + sg.begin); run.win.push_back(0); run.win.push_back(sg.end - sg.begin);
            run.tail.push_back(b.row_start[(size_t)j]); run.tail.push_back(nf);
            run.t0.push_back(t0_of[(size_t)j]); run.row0.push_back((int)((int64_t)i * k.T_pad)); run.len.push_back(nf);
            k.frames += nf; k.wave_frames += t0_of[(size_t)j]; k.attn_flops += 4.0 * (double)nf * nf * d;
        }
        run.chunks.push_back(k);
    }
    PCE_TRY(w2v_run_chunks(c, b, run));
    b.n_clips = n_seg;
    b.seg_plan[0] = (int64_t)sp.chunks.size(); b.seg_plan[1] = sp.rows_computed; b.seg_plan[2] = sp.rows_valid;
    return PCE_OK;
}

int pce_w2v_segments_plan(pce_ctx *c, int64_t *n_chunks, int64_t *rows_computed, int64_t *rows_valid)
{
    if (!c || !n_chunks || !rows_computed || !rows_valid) return PCE_E_INVALID;
    WhisperState::W2v &b = ws_of(c)->w2v;
    if (b.n_clips < 0 || b.seg_plan[0] < 0) return pce_fail(c, PCE_E_STATE, "pce_w2v_segments_plan: the latest run was no pce_w2v_run_segments");
    *n_chunks = b.seg_plan[0]; *rows_computed = b.seg_plan[1]; *rows_valid = b.seg_plan[2];
    return PCE_OK;
}

int pce_w2v_shape(pce_ctx *c, int32_t clip, int64_t *n_frames, int32_t *n_cols)
{
    if (!c || !n_frames || !n_cols) return PCE_E_INVALID;
    WhisperState::W2v &b = ws_of(c)->w2v;
    if (b.n_clips < 0) return pce_fail(c, PCE_E_STATE, "pce_w2v_shape before pce_w2v_run");
    if (clip < 0 || clip >= b.n_clips) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    *n_frames = b.n_frames[(size_t)clip]; *n_cols = b.n_cols;
    return PCE_OK;
}

int pce_w2v_fetch(pce_ctx *c, int32_t clip, float *log_probs)
{
    if (!c || !log_probs) return PCE_E_INVALID;
    WhisperState::W2v &b = ws_of(c)->w2v;
    if (b.n_clips < 0) return pce_fail(c, PCE_E_STATE, "pce_w2v_fetch before pce_w2v_run");
    if (clip < 0 || clip >= b.n_clips) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_FETCH(c, log_probs, b.em.as<float>() + b.row_start[(size_t)clip] * b.n_cols, (size_t)b.n_frames[(size_t)clip] * b.n_cols);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

int pce_w2v_device(pce_ctx *c, const float **d_emissions, const int64_t **h_row_start, const int32_t **h_n_frames, int32_t *n_cols)
{
    if (!c || !d_emissions || !h_row_start || !h_n_frames || !n_cols) return PCE_E_INVALID;
    WhisperState::W2v &b = ws_of(c)->w2v;
    if (b.n_clips < 0) return pce_fail(c, PCE_E_STATE, "pce_w2v_device before pce_w2v_run");
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_HIP(c, hipStreamSynchronize(c->stream));                  // the emissions are complete when the pointer is handed out
    *d_emissions = b.em.as<float>(); *h_row_start = b.row_start.data(); *h_n_frames = b.n_frames.data(); *n_cols = b.n_cols;
    return PCE_OK;
}

// ---- stage self-tests: the three new stages through the run's own launches -----------------------------------------------------------------
int pce_selftest_w2v_wave(pce_ctx *c, const int16_t *pcm, int64_t n_samples, int32_t window_samples, int32_t context_samples, int32_t feat_norm, int32_t C,
                          int32_t stride, const float *w, const float *bias, const float *gamma, const float *beta, uint16_t *out)
{
    if (!c || !pcm || !w || !gamma || !beta || !out || n_samples < 1 || window_samples < 1 || context_samples < 0 || (feat_norm != 0 && feat_norm != 1))
        return PCE_E_INVALID;
    if (C <= 0 || C % 64 || C > WV_C_MAX || stride < 1 || stride > WV_STRIDE_MAX)
        return pce_fail(c, PCE_E_LIMIT, "selftest waveform layer: %d channels at stride %d (channels %% 64 == 0 and <= %d, stride <= %d)", C, stride, WV_C_MAX, WV_STRIDE_MAX);
    PCE_HIP(c, hipSetDevice(c->device));
    const int64_t L = (int64_t)window_samples + 2 * (int64_t)context_samples, T0 = L >= WV_K0 ? (L - WV_K0) / stride + 1 : 0;
    int64_t n_win, keep;
    pce_w2v_window_plan(n_samples, window_samples, context_samples, &n_win, &keep);
    if (T0 == 0) return PCE_OK;                                                 // shorter than one tap window: no frames
    if (T0 > INT32_MAX / 2 || n_win > 65535) return pce_fail(c, PCE_E_LIMIT, "selftest waveform layer: too many frames or windows");
    std::vector<int64_t> tab;
    for (int64_t j = 0; j < n_win; j++) { tab.push_back(0); tab.push_back(j * window_samples - context_samples); tab.push_back(n_samples); }
    return w2v_selftest_wave(c, pcm, n_samples, tab, std::vector<int>((size_t)n_win, (int)T0), feat_norm, C, stride, w, bias, gamma, beta, out);
}

int pce_selftest_w2v_lngelu(pce_ctx *c, const uint16_t *x, int32_t rows, int32_t C, const float *w, const float *b, float eps, int32_t gelu, uint16_t *out)
{
    if (!c || !x || !w || !b || !out || rows < 1) return PCE_E_INVALID;
    if (C < 8 || C % 8 || C > LN_D_MAX) return pce_fail(c, PCE_E_LIMIT, "selftest LayerNorm + GELU: C = %d (need C %% 8 == 0, C <= %d)", C, LN_D_MAX);
    PCE_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)rows * C;
    DevBuf dx, dw, db;
    PCE_UPLOAD(c, dx, x, n); PCE_UPLOAD(c, dw, w, (size_t)C); PCE_UPLOAD(c, db, b, (size_t)C);
    w2v_launch_ln16(c, gelu != 0, dx.as<op_t>(), dw.as<float>(), db.as<float>(), rows, C, eps, dx.as<op_t>());      // in place, as the run launches it
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, out, dx.p, n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

int pce_selftest_w2v_posconv(pce_ctx *c, const float *x, int32_t n_win, int32_t T, int32_t d, int32_t groups, const uint16_t *w, const float *bias, float *out)
{
    if (!c || !x || !w || !bias || !out || n_win < 1 || n_win > 65535 || T < 1) return PCE_E_INVALID;
    if (!w2v_posconv_fits(d, groups) || d % 4) return pce_fail(c, PCE_E_LIMIT, "selftest positional convolution: d = %d in %d groups (16, 32, 48 or 64 columns per group)", d, groups);
    const std::vector<int32_t> len((size_t)n_win, T);               // T frames in every window
    return PCE_BUILD_NS::pce_selftest_w2v_posconv_segments(c, x, n_win, len.data(), T, d, groups, w, bias, out);
}

// ... and the two stages with unequal frame counts, as pce_w2v_run_segments launches them.  _wave_segments: item i is samples
// [seg[2 i], seg[2 i + 1]) of ONE clip, run on max(its samples, min_samples); out as w2v_selftest_wave lays it out.  _posconv_segments: n_win
// windows of len[i] <= T frames in slots of T rows.
int pce_selftest_w2v_wave_segments(pce_ctx *c, const int16_t *pcm, int64_t n_samples, const int64_t *seg, int32_t n_seg, int32_t min_samples, int32_t feat_norm,
                                   int32_t C, int32_t stride, const float *w, const float *bias, const float *gamma, const float *beta, uint16_t *out)
{
    if (!c || !pcm || !seg || !w || !gamma || !beta || !out || n_samples < 1 || n_seg < 1 || n_seg > 65535 || min_samples < 0 || (feat_norm != 0 && feat_norm != 1))
        return PCE_E_INVALID;
    if (C <= 0 || C % 64 || C > WV_C_MAX || stride < 1 || stride > WV_STRIDE_MAX)
        return pce_fail(c, PCE_E_LIMIT, "selftest waveform layer: %d channels at stride %d (channels %% 64 == 0 and <= %d, stride <= %d)", C, stride, WV_C_MAX, WV_STRIDE_MAX);
    PCE_HIP(c, hipSetDevice(c->device));
    std::vector<int64_t> tab;
    std::vector<int> t0;
    for (int i = 0; i < n_seg; i++) {
        const int64_t b0 = seg[2 * i], e0 = seg[2 * i + 1];
        if (b0 < 0 || b0 > e0 || e0 > n_samples) return pce_fail(c, PCE_E_INVALID, "selftest waveform layer: segment %d outside the clip", i);
        const int64_t L = std::max<int64_t>(e0 - b0, min_samples), T0 = L >= WV_K0 ? (L - WV_K0) / stride + 1 : 0;
        if (T0 < 1 || T0 > INT32_MAX / 2) return pce_fail(c, PCE_E_LIMIT, "selftest waveform layer: segment %d gives %lld frames", i, (long long)T0);
        tab.push_back(b0); tab.push_back(0); tab.push_back(e0 - b0);
        t0.push_back((int)T0);
    }
    return w2v_selftest_wave(c, pcm, n_samples, tab, t0, feat_norm, C, stride, w, bias, gamma, beta, out);
}

int pce_selftest_w2v_posconv_segments(pce_ctx *c, const float *x, int32_t n_win, const int32_t *len, int32_t T, int32_t d, int32_t groups, const uint16_t *w,
                                      const float *bias, float *out)
{
    if (!c || !x || !len || !w || !bias || !out || n_win < 1 || n_win > 65535 || T < 1) return PCE_E_INVALID;
    if (!w2v_posconv_fits(d, groups) || d % 4) return pce_fail(c, PCE_E_LIMIT, "selftest positional convolution: d = %d in %d groups (16, 32, 48 or 64 columns per group)", d, groups);
    double frames = 0.0;
    for (int i = 0; i < n_win; i++) {
        if (len[i] < 1 || len[i] > T) return pce_fail(c, PCE_E_INVALID, "selftest positional convolution: window %d holds %d of %d frames", i, len[i], T);
        frames += len[i];
    }
    PCE_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_win * T * d, nw = (size_t)d * PC_TAPS * (d / groups);
    DevBuf dx, dl, dw, db, dout;
    PCE_UPLOAD(c, dx, x, n); PCE_UPLOAD(c, dl, len, (size_t)n_win); PCE_UPLOAD(c, dw, w, nw); PCE_UPLOAD(c, db, bias, (size_t)d);
    PCE_ZERO(float, c, dout, n);
    w2v_launch_posconv(c, dx.as<float>(), dw.as<op_t>(), db.as<float>(), dl.as<int>(), frames, T, d, groups, n_win, dout.as<float>());
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, out, dout.p, n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

} // namespace PCE_BUILD_NS
