// pce_crepe.hip -- CREPE pitch tracking of the resident batch (include/pce.h, "CREPE pitch tracking"): what
//   torchcrepe.predict(audio, sr, hop, fmin, fmax, model, batch_size=4096, return_periodicity=True)
// computes in Code/Pipeline/evaluate_voice.ipynb (extract_f0_torchcrepe).  torchcrepe is third party and absent: restated from its published
// implementation (core.py preprocess / infer / postprocess, model.py, decode.py viterbi; librosa sequence.viterbi), parity unpinned;
// tests/crepe_restatement.py is the float64 restatement the tests compare with.
//
// k_crepe_frames      one wavefront per frame: int16 samples -> mean / unbiased std from exact integer sums -> fp16 into block 1's operand image
//                     (1024 values behind 254 zeros; no float copy of the audio exists).
// k_crepe_conv1       block 1 (C_in = 1, stride 4, 512 taps): the frame in LDS, A fragments are 8-byte LDS reads at x[4 m + k], B fragments come
//                     from the weights directly (1 MiB at most: L2); one workgroup = one frame x 64 output channels.
// k_crepe_conv<BN>    blocks 2-6 as GEMMs C[m][n] = sum_k A[m][k] W[n][k] over padded time-major images: row m = (frame, t) starts at
//                     image[frame][t * C_in] and is K = 64 C_in contiguous values (lda = C_in < K: the rows overlap).  128 x BN x 64 tiles, operand
//                     tiles by LDS-DMA into an XOR-swizzled two-stage ring, v_mfma_f32_16x16x32_f16.
// Both conv kernels share the epilogue: relu(acc + bias) * scale + shift per element, the maximum of rows 2 m and 2 m + 1 (they sit in one lane's
// accumulator registers), fp16, staged per wave in LDS and written as 16-byte pieces of row m of the NEXT block's padded image.  The pad rows of the
// images are cleared once per pce_crepe_run; no kernel writes them.
// k_crepe_classifier  eight frames per workgroup, one wavefront per pitch bin at a time: fp32 weights, fp32 FMA in a fixed order, sigmoid.
// k_crepe_logprob     one wavefront per frame: mask, softmax over the 360 sigmoid outputs (as torchcrepe does), log(p + tiny) in fp64; the arg-max decoder.
// k_crepe_viterbi     one workgroup per clip, modelled on k_pyin_viterbi: 360 states, the 25-wide band from a table in LDS, out-of-band
//                     predecessors (log(0 + tiny)) through prefix / suffix maxima of value + log(tiny) (first index on ties: librosa's dense argmax),
//                     fp64 scores, back-pointers in HBM, back-tracking by one lane.
// k_crepe_gather      f0 (table of the 360 bin frequencies) and periodicity = salience[t][bin].
// A frame's arithmetic never depends on which chunk, tile or batch it is in: kernels are chosen by N and K alone.
#include "pce_internal.h"
#include "pce_wave.h"
#include <cfloat>
#include <cmath>

namespace {

typedef _Float16 h16;
typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 h16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int CR_WIN = 1024, CR_BINS = PCE_CREPE_BINS, CR_RATE = 16000;
constexpr int CR_PAD1 = 254, CR_IMG1 = 1536;              // block 1's image row: 254 zeros, 1024 values, 254 zeros, 4 of slack (16-byte rows)
constexpr int CR_TAPS1 = 512, CR_T1 = 256;                // block 1: taps, conv rows per frame (stride 4)
constexpr int CR_TAPS = 64, CR_PADL = 31, CR_PADR = 32;   // blocks 2-6
constexpr int CR_HALF = 12, CR_BAND = 2 * CR_HALF + 1;    // transition max(12 - |i - j|, 0): the entries at +-12 are zeros already
constexpr double CR_CENTS0 = 1997.3794084376191;
constexpr int CR_BM = 128, CR_BK = 64;

__device__ __forceinline__ f32x4 mfma_f16(h16x8 a, h16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ int cr_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }   // 16-byte chunks of a 128-byte LDS row

// __syncthreads() for the kernels marked PCE_NO_PK_F32: the header's function is not force-inlined, so under the attribute it stays a call
__device__ __forceinline__ void cr_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ void k_crepe_f32_to_f16(const float *__restrict__ in, h16 *__restrict__ out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (h16)in[i];
}

// ---------------------------------------------------------------------------------------------------------------
// frames
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_crepe_frames(const int16_t *__restrict__ pcm, const int64_t *__restrict__ clip_off,
                                                      const int64_t *__restrict__ frame_off, int n_clips, int hop, int64_t g0, int n_frames,
                                                      h16 *__restrict__ img1)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int f = (int)blockIdx.x * 4 + wv;
    if (f >= n_frames) return;
    const int64_t g = g0 + f;
    int lo = 0, hi = n_clips;                                   // the clip of global frame g: frame_off[lo] <= g < frame_off[lo + 1]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (frame_off[mid] <= g) lo = mid; else hi = mid; }
    const int64_t c0 = clip_off[lo], len = clip_off[lo + 1] - c0;
    const int64_t s0 = (g - frame_off[lo]) * hop - CR_WIN / 2;
    // sums of the int16 values and of their squares: integers below 2^41, exact in fp64 in any order
    int v[CR_WIN / 64];
    double S = 0.0, Q = 0.0;
#pragma unroll
    for (int k = 0; k < CR_WIN / 64; k++) {
        const int64_t s = s0 + lane + 64 * k;
        v[k] = (s >= 0 && s < len) ? (int)pcm[c0 + s] : 0;
        S += (double)v[k]; Q += (double)v[k] * (double)v[k];
    }
    S = wave_xor_sum(S); Q = wave_xor_sum(Q);
    // x = v / 32768: (x - mean(x)) / max(1e-10, std(x)), std with divisor N - 1
    const double mean = S / CR_WIN;
    double var = (Q - S * S / CR_WIN) / (CR_WIN - 1);
    if (var < 0.0) var = 0.0;
    const double sd = sqrt(var) / 32768.0;
    const double den = (sd > 1e-10 ? sd : 1e-10) * 32768.0;
    h16 *dst = img1 + (int64_t)f * CR_IMG1 + CR_PAD1;
#pragma unroll
    for (int k = 0; k < CR_WIN / 64; k++) dst[lane + 64 * k] = (h16)(float)(((double)v[k] - mean) / den);
}

// ---------------------------------------------------------------------------------------------------------------
// the shared epilogue: one wave's MI x NJ accumulator blocks (rows w_row0 + 16 i + 4 (lane >> 4) + r, columns w_col0 + 16 j + (lane & 15))
// ---------------------------------------------------------------------------------------------------------------
template <int MI, int NJ>
__device__ __forceinline__ void crepe_pool_to_lds(const f32x4 (&acc)[MI][NJ], const float *__restrict__ bias, const float *__restrict__ scale,
                                                  const float *__restrict__ shift, int col0 /* global column of j = 0, lane & 15 == 0 */, int lane,
                                                  h16 *wt /* this wave's [MI * 8][NJ * 16 + 8] */)
{
    constexpr int LD = NJ * 16 + 8;
    const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int n = col0 + j * 16 + fr;
        const float b = bias[n], sc = scale[n], sh = shift[n];
#pragma unroll
        for (int i = 0; i < MI; i++) {
            float y[4];
#pragma unroll
            for (int r = 0; r < 4; r++) y[r] = fmaxf(acc[i][j][r] + b, 0.f) * sc + sh;       // ReLU, then BatchNorm: scale may be negative
            wt[(i * 8 + fq * 2) * LD + j * 16 + fr] = (h16)fmaxf(y[0], y[1]);                // the pool compares values after BatchNorm
            wt[(i * 8 + fq * 2 + 1) * LD + j * 16 + fr] = (h16)fmaxf(y[2], y[3]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// block 1
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) PCE_NO_PK_F32 void k_crepe_conv1(const h16 *__restrict__ img1, const h16 *__restrict__ W /* [N][512] */,
                                                                    const float *__restrict__ bias, const float *__restrict__ scale,
                                                                    const float *__restrict__ shift, int N, h16 *__restrict__ out, int64_t out_fstride,
                                                                    int out_row_off)
{
    __shared__ __attribute__((aligned(16))) h16 xs[CR_IMG1];
    __shared__ __attribute__((aligned(16))) h16 ot[4][32 * 72];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f = blockIdx.y, n0 = (int)blockIdx.x * 64;
    if (tid < CR_IMG1 / 8) reinterpret_cast<uint4 *>(xs)[tid] = reinterpret_cast<const uint4 *>(img1 + (int64_t)f * CR_IMG1)[tid];
    cr_sync();
    const int fr = lane & 15, fq = lane >> 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const h16 *wp = W + (int64_t)(n0 + fr) * CR_TAPS1 + 8 * fq;
#pragma unroll 4
    for (int kk = 0; kk < CR_TAPS1; kk += 32) {
        h16x8 a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; j++) b[j] = *reinterpret_cast<const h16x8 *>(wp + (int64_t)j * 16 * CR_TAPS1 + kk);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const h16 *p = xs + 4 * (wv * 64 + i * 16 + fr) + kk + 8 * fq;       // 4 m + k <= 4 * 255 + 511 = 1531; 8-byte aligned
            const h16x4 l = *reinterpret_cast<const h16x4 *>(p), h = *reinterpret_cast<const h16x4 *>(p + 4);
            a[i] = h16x8{l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = mfma_f16(a[i], b[j], acc[i][j]);
    }
    crepe_pool_to_lds<4, 4>(acc, bias, scale, shift, n0, lane, ot[wv]);
    cr_sync();
    // the wave's 32 pooled rows (rows wv * 32 .. of the frame's 128) x 64 columns: 8 lanes x 16 bytes per row
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int prow = p * 8 + (lane >> 3), ch = lane & 7;
        const uint4 val = *reinterpret_cast<const uint4 *>(&ot[wv][prow * 72 + ch * 8]);
        *reinterpret_cast<uint4 *>(out + (int64_t)f * out_fstride + (int64_t)(out_row_off + wv * 32 + prow) * N + n0 + ch * 8) = val;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// blocks 2-6
// ---------------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const h16 *A; int64_t in_fstride; int c_in, t_shift /* log2 T_in */;
    const h16 *W; const float *bias, *scale, *shift;
    int M /* n_frames * T_in */, N, K;
    h16 *out; int64_t out_fstride; int out_row_off;
};

// rows [row0, row0 + ROWS) x 64 k of an operand as LDS-DMA: one wave instruction moves 8 rows of 128 bytes; the 16-byte chunks of a row are
// XOR-swizzled on the GLOBAL side (the LDS side of the DMA is fixed: base + 16 * lane), and again when the fragments are read
template <int ROWS, bool IS_A>
__device__ __forceinline__ void crepe_stage(const ConvArgs &g, int row0, int k0, h16 *lds_tile, int wv, int lane)
{
#pragma unroll
    for (int q = 0; q < (ROWS / 8 + 3) / 4; q++) {
        const int inst = q * 4 + wv;
        if (ROWS / 8 % 4 != 0 && inst >= ROWS / 8) break;                    // (wave-uniform)
        const int row = inst * 8 + (lane >> 3);
        const int c = cr_swz(row, lane & 7);
        const h16 *src;
        if (IS_A) {
            int r = row0 + row; if (r > g.M - 1) r = g.M - 1;                // rows past the end repeat the last row; their results are not stored
            const int fr = r >> g.t_shift, t = r & ((1 << g.t_shift) - 1);
            src = g.A + (int64_t)fr * g.in_fstride + (int64_t)t * g.c_in + k0 + c * 8;      // t c_in + K <= (T_in + 63) c_in = in_fstride
        } else {
            src = g.W + (int64_t)(row0 + row) * g.K + k0 + c * 8;            // row0 + row < N: N % BN == 0
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(lds_tile + inst * 8 * CR_BK), 16, 0, 0);
    }
}

// 4 waves as WR (M) x WC (N); BN = 128: 2 x 2 waves of 64 x 64, BN = 16: 4 x 1 waves of 32 x 16
template <int BN, int WR, int WC>
__global__ __launch_bounds__(256, 2) PCE_NO_PK_F32 void k_crepe_conv(ConvArgs g)
{
    constexpr int WROWS = CR_BM / WR, WCOLS = BN / WC, MI = WROWS / 16, NJ = WCOLS / 16;
    constexpr int STAGE = (CR_BM + BN) * CR_BK;
    constexpr int WT = (WROWS / 2) * (WCOLS + 8);                                 // a wave's pooled tile
    static_assert(4 * WT <= 2 * STAGE, "the pooled tiles reuse the operand ring");
    __shared__ __attribute__((aligned(1024))) h16 smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = wv / WC, wc = wv % WC;
    const int n0 = (int)blockIdx.x * BN, m0 = (int)blockIdx.y * CR_BM;
    const int fr = lane & 15, fq = lane >> 4;
    f32x4 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < NJ; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = g.K / CR_BK;
    crepe_stage<CR_BM, true>(g, m0, 0, smem, wv, lane);
    crepe_stage<BN, false>(g, n0, 0, smem + CR_BM * CR_BK, wv, lane);
    for (int kt = 0; kt < nk; kt++) {
        const h16 *sA = smem + (kt & 1) * STAGE, *sB = sA + CR_BM * CR_BK;
        __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0): this wave's share of tile kt has landed
        __builtin_amdgcn_s_barrier();                       // ... everyone's has, and everyone is done reading tile kt - 1
        if (kt + 1 < nk) {
            h16 *nx = smem + ((kt + 1) & 1) * STAGE;
            crepe_stage<CR_BM, true>(g, m0, (kt + 1) * CR_BK, nx, wv, lane);
            crepe_stage<BN, false>(g, n0, (kt + 1) * CR_BK, nx + CR_BM * CR_BK, wv, lane);
        }
#pragma unroll
        for (int kk = 0; kk < CR_BK; kk += 32) {
            h16x8 a[MI], b[NJ];
#pragma unroll
            for (int i = 0; i < MI; i++) {
                const int row = wr * WROWS + i * 16 + fr;
                a[i] = *reinterpret_cast<const h16x8 *>(&sA[row * CR_BK + cr_swz(row, (kk >> 3) + fq) * 8]);
            }
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                const int row = wc * WCOLS + j * 16 + fr;
                b[j] = *reinterpret_cast<const h16x8 *>(&sB[row * CR_BK + cr_swz(row, (kk >> 3) + fq) * 8]);
            }
#pragma unroll
            for (int i = 0; i < MI; i++)
#pragma unroll
                for (int j = 0; j < NJ; j++) acc[i][j] = mfma_f16(a[i], b[j], acc[i][j]);
        }
    }
    cr_sync();                                         // every wave is done with the operand ring
    h16 *wt = smem + wv * WT;
    crepe_pool_to_lds<MI, NJ>(acc, g.bias, g.scale, g.shift, n0 + wc * WCOLS, lane, wt);
    cr_sync();
    constexpr int LPR = WCOLS / 8;                           // 16-byte pieces per pooled row
    const int t_out_shift = g.t_shift - 1;
    for (int idx = lane; idx < (WROWS / 2) * LPR; idx += 64) {
        const int prow = idx / LPR, ch = idx % LPR;
        const int R = (m0 + wr * WROWS) / 2 + prow;          // pooled row over all frames of the chunk
        if (2 * R >= g.M) continue;
        const int frm = R >> t_out_shift, t = R & ((1 << t_out_shift) - 1);
        const uint4 val = *reinterpret_cast<const uint4 *>(&wt[prow * (WCOLS + 8) + ch * 8]);
        *reinterpret_cast<uint4 *>(g.out + (int64_t)frm * g.out_fstride + (int64_t)(g.out_row_off + t) * g.N + n0 + wc * WCOLS + ch * 8) = val;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// classifier + sigmoid
// ---------------------------------------------------------------------------------------------------------------
constexpr int CL_FRAMES = 8;
__global__ __launch_bounds__(256) PCE_NO_PK_F32 void k_crepe_classifier(const h16 *__restrict__ emb, int E, const float *__restrict__ W /* [360][E] */,
                                                                         const float *__restrict__ bias, int n_frames, float *__restrict__ P /* [n_frames][360] */)
{
    extern __shared__ __attribute__((aligned(16))) h16 xs[];           // [CL_FRAMES][E]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f0 = (int)blockIdx.x * CL_FRAMES;
    for (int i = tid; i < CL_FRAMES * E / 8; i += 256) {
        const int f = (i * 8) / E;
        reinterpret_cast<uint4 *>(xs)[i] = f0 + f < n_frames ? reinterpret_cast<const uint4 *>(emb + (int64_t)f0 * E)[i] : make_uint4(0, 0, 0, 0);
    }
    cr_sync();
    for (int b = wv; b < CR_BINS; b += 4) {
        float acc[CL_FRAMES];
#pragma unroll
        for (int f = 0; f < CL_FRAMES; f++) acc[f] = 0.f;
        for (int k = lane * 4; k < E; k += 256) {                        // E % 256 == 0: a lane's terms in ascending k, then the butterfly
            const float4 w = *reinterpret_cast<const float4 *>(W + (int64_t)b * E + k);
#pragma unroll
            for (int f = 0; f < CL_FRAMES; f++) {
                const h16x4 e = *reinterpret_cast<const h16x4 *>(xs + f * E + k);
                acc[f] = fmaf(w.x, (float)e[0], acc[f]); acc[f] = fmaf(w.y, (float)e[1], acc[f]);
                acc[f] = fmaf(w.z, (float)e[2], acc[f]); acc[f] = fmaf(w.w, (float)e[3], acc[f]);
            }
        }
        const float bb = bias[b];
#pragma unroll
        for (int f = 0; f < CL_FRAMES; f++) {
            const float z = wave_xor_sum(acc[f]) + bb;
            if (lane == f && f0 + f < n_frames) P[(int64_t)(f0 + f) * CR_BINS + b] = 1.f / (1.f + expf(-z));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// decoding
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_crepe_logprob(const float *__restrict__ P, int64_t total, int lo, int hi, double tiny, double c0 /* log(tiny) */,
                                                       double *__restrict__ logp /* or nullptr */, int *__restrict__ amax)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= total) return;
    constexpr int R = (CR_BINS + 63) / 64;
    float x[R];
    float mx = -INFINITY; int mi = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int b = lane + 64 * r;
        const bool in = b >= lo && b < hi;
        x[r] = in ? P[g * CR_BINS + b] : -INFINITY;
        if (in && x[r] > mx) { mx = x[r]; mi = b; }                  // ascending b within the lane: the first maximum
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 64); const int oi = __shfl_xor(mi, o, 64);
        if (ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; }
    }
    if (lane == 0) amax[g] = mi == 0x7fffffff ? lo : mi;            // (a frame of NaN compares false everywhere: the first unmasked bin, in range for the gather)
    if (!logp) return;
    double e[R], s = 0.0;
#pragma unroll
    for (int r = 0; r < R; r++) { e[r] = x[r] == -INFINITY ? 0.0 : exp((double)x[r] - (double)mx); s += e[r]; }
    s = wave_xor_sum(s);
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int b = lane + 64 * r;
        if (b < CR_BINS) logp[g * CR_BINS + b] = x[r] == -INFINITY ? c0 : log(e[r] / s + tiny);
    }
}

constexpr int CV_THREADS = 384;
struct BestIdx { double v; int i; };

__global__ __launch_bounds__(CV_THREADS) void k_crepe_viterbi(const int64_t *__restrict__ frame_off, const double *__restrict__ logp,
                                                             const double *__restrict__ lt_g /* [CR_BAND][360]: [e + 12][i] = log(T[i][i + e] + tiny) */,
                                                             double c0, double log_pinit, unsigned short *__restrict__ ptr, int *__restrict__ bins)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *lt = lds;                                   // [CR_BAND][360]
    double *V = lt + CR_BAND * CR_BINS;                 // [360]
    double *pv = V + CR_BINS;                           // [2][360] prefix maxima of V + c0 (double buffered scan)
    double *sv = pv + 2 * CR_BINS;                      // [2][360] suffix maxima
    int *pi = reinterpret_cast<int *>(sv + 2 * CR_BINS);   // [2][360]
    int *si = pi + 2 * CR_BINS;                         // [2][360]
    const int j = threadIdx.x;
    const int64_t f0 = frame_off[blockIdx.x], T = frame_off[blockIdx.x + 1] - f0;
    if (T <= 0) return;
    for (int i = j; i < CR_BAND * CR_BINS; i += CV_THREADS) lt[i] = lt_g[i];
    if (j < CR_BINS) V[j] = logp[f0 * CR_BINS + j] + log_pinit;
    __syncthreads();
    for (int64_t t = 1; t < T; t++) {
        // out-of-band predecessors all carry log(0 + tiny): the first maximum of V[i] + c0 over a prefix / a suffix of the states
        if (j < CR_BINS) { const double s = V[j] + c0; pv[j] = s; sv[j] = s; pi[j] = j; si[j] = j; }
        __syncthreads();
        int cur = 0;
        for (int o = 1; o < CR_BINS; o <<= 1) {
            if (j < CR_BINS) {
                BestIdx a{pv[cur * CR_BINS + j], pi[cur * CR_BINS + j]};
                if (j >= o) { const double lv = pv[cur * CR_BINS + j - o]; if (!(a.v > lv)) { a.v = lv; a.i = pi[cur * CR_BINS + j - o]; } }   // the left part wins ties
                pv[(cur ^ 1) * CR_BINS + j] = a.v; pi[(cur ^ 1) * CR_BINS + j] = a.i;
                BestIdx b{sv[cur * CR_BINS + j], si[cur * CR_BINS + j]};
                if (j + o < CR_BINS) { const double rv = sv[cur * CR_BINS + j + o]; if (rv > b.v) { b.v = rv; b.i = si[cur * CR_BINS + j + o]; } }
                sv[(cur ^ 1) * CR_BINS + j] = b.v; si[(cur ^ 1) * CR_BINS + j] = b.i;
            }
            __syncthreads();
            cur ^= 1;
        }
        double nv = 0.0;
        if (j < CR_BINS) {
            // candidates in index order, strict '>' keeps the first maximum (np.argmax)
            double best = -INFINITY; int bi = 0;
            if (j - CR_HALF - 1 >= 0) { best = pv[cur * CR_BINS + j - CR_HALF - 1]; bi = pi[cur * CR_BINS + j - CR_HALF - 1]; }
#pragma unroll
            for (int e = -CR_HALF; e <= CR_HALF; e++) {
                const int i = j + e;                                   // predecessor i, target j = i - (-e)
                if (i >= 0 && i < CR_BINS) {
                    const double c = V[i] + lt[(CR_HALF - e) * CR_BINS + i];      // log(T[i][j] + tiny), j - i = -e
                    if (c > best) { best = c; bi = i; }
                }
            }
            if (j + CR_HALF + 1 < CR_BINS) {
                const double c = sv[cur * CR_BINS + j + CR_HALF + 1];
                if (c > best) { best = c; bi = si[cur * CR_BINS + j + CR_HALF + 1]; }
            }
            nv = logp[(f0 + t) * CR_BINS + j] + best;
            ptr[(f0 + t) * CR_BINS + j] = (unsigned short)bi;
        }
        __syncthreads();
        if (j < CR_BINS) V[j] = nv;
        __syncthreads();
    }
    if (j == 0) {
        double best = V[0]; int bi = 0;
        for (int s = 1; s < CR_BINS; s++) if (V[s] > best) { best = V[s]; bi = s; }
        int *st = bins + f0;
        st[T - 1] = bi;
        for (int64_t t = T - 2; t >= 0; t--) { bi = ptr[(f0 + t + 1) * CR_BINS + bi]; st[t] = bi; }
    }
}

__global__ void k_crepe_gather(const int *__restrict__ bins, const float *__restrict__ P, const double *__restrict__ ftab, int64_t total,
                               double *__restrict__ f0, float *__restrict__ per)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const int b = bins[g];
    f0[g] = ftab[b];
    per[g] = P[g * CR_BINS + b];
}

// ---------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------
int crepe_t_in(int block) { return block == 1 ? CR_WIN : 128 >> (block - 2); }          // rows a block's convolution produces per frame (block 1: 256 after the stride)
int64_t crepe_img_elems(const int *c_in, int i /* img index 1..5: input of block i + 1 */) { return (int64_t)(crepe_t_in(i + 1) + CR_PADL + CR_PADR) * c_in[i]; }

int crepe_dims_ok(pce_ctx *c, const int *c_in, const int *c_out)
{
    bool ok = c_in[0] == 1 && c_out[0] > 0 && c_out[0] % 64 == 0;
    for (int i = 1; i < 6; i++) ok = ok && c_in[i] == c_out[i - 1];
    for (int i = 0; i < 6; i++) ok = ok && c_out[i] > 0 && c_out[i] % 16 == 0 && c_out[i] <= 8192;
    const int E = 4 * c_out[5];
    ok = ok && E % 256 == 0 && E <= 4096;
    return ok ? PCE_OK : pce_fail(c, PCE_E_LIMIT, "unsupported CREPE widths (c_out[0] %% 64 == 0, every c_out %% 16 == 0, 4 c_out[5] %% 256 == 0 and <= 4096)");
}

// one block as the product launches it; the kernel follows N alone
int crepe_launch_block(pce_ctx *c, int block, const h16 *in, int c_in, int N, const h16 *W, const float *bss /* bias | scale | shift */, h16 *out,
                       int64_t out_fstride, int out_row_off, int n_frames)
{
    if (block == 1) {
        const double flops = 2.0 * CR_T1 * CR_TAPS1 * (double)N * n_frames;
        KernelTimer t(c, PCE_K_CREPE_CONV1, nullptr, flops);
        hipLaunchKernelGGL(k_crepe_conv1, dim3((unsigned)(N / 64), (unsigned)n_frames), dim3(256), 0, c->stream, in, W, bss, bss + N, bss + 2 * N, N, out,
                           out_fstride, out_row_off);
        return PCE_OK;
    }
    const int T = crepe_t_in(block);
    ConvArgs g{};
    g.A = in; g.in_fstride = (int64_t)(T + CR_PADL + CR_PADR) * c_in; g.c_in = c_in;
    g.t_shift = 0; while ((1 << g.t_shift) < T) g.t_shift++;
    g.W = W; g.bias = bss; g.scale = bss + N; g.shift = bss + 2 * N;
    g.M = n_frames * T; g.N = N; g.K = CR_TAPS * c_in;
    g.out = out; g.out_fstride = out_fstride; g.out_row_off = out_row_off;
    const double flops = 2.0 * (double)g.M * g.N * g.K;
    KernelTimer t(c, block == 2 ? PCE_K_CREPE_CONV2 : PCE_K_CREPE_CONV, nullptr, flops);
    const unsigned gy = (unsigned)div_up(g.M, CR_BM);
    if (N % 128 == 0) hipLaunchKernelGGL((k_crepe_conv<128, 2, 2>), dim3((unsigned)(N / 128), gy), dim3(256), 0, c->stream, g);
    else hipLaunchKernelGGL((k_crepe_conv<16, 4, 1>), dim3((unsigned)(N / 16), gy), dim3(256), 0, c->stream, g);
    return PCE_OK;
}

int upload_f16(pce_ctx *c, const float *src, int64_t n, DevBuf &dst, DevBuf &tmp)
{
    PCE_UPLOAD(c, tmp, src, (size_t)n);
    PCE_HIP(c, dst.reserve(sizeof(h16) * (size_t)n + 64));
    hipLaunchKernelGGL(k_crepe_f32_to_f16, dim3(1024), dim3(256), 0, c->stream, tmp.as<float>(), dst.as<h16>(), n);
    PCE_HIP(c, hipGetLastError());
    PCE_HIP(c, hipStreamSynchronize(c->stream));       // tmp is reused by the next tensor
    return PCE_OK;
}


// buffers of the decoding for `total` frames of `n_clips` clips (cr.off filled), and its tables
int crepe_decode_prepare(pce_ctx *c, int32_t n_clips, int64_t total)
{
    auto &cr = c->cr;
    PCE_HIP(c, cr.P.reserve(sizeof(float) * (size_t)total * CR_BINS));
    PCE_HIP(c, cr.amax.reserve(sizeof(int) * (size_t)total));
    PCE_HIP(c, cr.bins.reserve(sizeof(int) * (size_t)total));
    PCE_HIP(c, cr.f0.reserve(sizeof(double) * (size_t)total));
    PCE_HIP(c, cr.per.reserve(sizeof(float) * (size_t)total));
    // tables: the 360 bin frequencies, then the log transition band [e + 12][i] = log(T[i][i + e] + tiny), rows of T normalised to 1
    const double tiny = DBL_MIN;
    std::vector<double> tab((size_t)CR_BINS + (size_t)CR_BAND * CR_BINS);
    for (int b = 0; b < CR_BINS; b++) tab[(size_t)b] = 10.0 * std::exp2((20.0 * b + CR_CENTS0) / 1200.0);
    for (int i = 0; i < CR_BINS; i++) {
        double rs = 0.0;
        for (int j2 = 0; j2 < CR_BINS; j2++) { const int d = i > j2 ? i - j2 : j2 - i; rs += d < CR_HALF ? (double)(CR_HALF - d) : 0.0; }
        for (int e = -CR_HALF; e <= CR_HALF; e++) {
            const int d = e < 0 ? -e : e, j2 = i + e;
            const double p = (j2 >= 0 && j2 < CR_BINS && d < CR_HALF) ? (double)(CR_HALF - d) / rs : 0.0;
            tab[(size_t)CR_BINS + (size_t)(e + CR_HALF) * CR_BINS + i] = std::log(p + tiny);
        }
    }
    PCE_UPLOAD(c, cr.tab, tab);
    PCE_UPLOAD(c, cr.doff, cr.off.data(), (size_t)n_clips + 1);
    PCE_HIP(c, hipStreamSynchronize(c->stream));                 // `tab` is a source of an asynchronous copy
    return PCE_OK;
}

// mask, log-softmax / arg-max, Viterbi, gather: cr.P [total][360] -> bins, f0, periodicity
int crepe_decode(pce_ctx *c, int32_t n_clips, int64_t total, int lo, int hi, int decoder)
{
    auto &cr = c->cr;
    const double tiny = DBL_MIN, c0 = std::log(tiny);
    const bool vit = decoder == 0;
    if (vit) {
        PCE_HIP(c, cr.logp.reserve(sizeof(double) * (size_t)total * CR_BINS));
        PCE_HIP(c, cr.ptr.reserve(sizeof(unsigned short) * (size_t)total * CR_BINS));
    }
    {
        KernelTimer t(c, PCE_K_CREPE_DECODE);
        hipLaunchKernelGGL(k_crepe_logprob, dim3((unsigned)div_up(total, 4)), dim3(256), 0, c->stream, cr.P.as<float>(), total, lo, hi,
                           tiny, c0, vit ? cr.logp.as<double>() : nullptr, cr.amax.as<int>());
    }
    if (vit) {
        const size_t lds = sizeof(double) * (size_t)(CR_BAND * CR_BINS + 5 * CR_BINS) + sizeof(int) * (size_t)(4 * CR_BINS);
        PCE_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_crepe_viterbi), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        KernelTimer t(c, PCE_K_CREPE_VITERBI);
        hipLaunchKernelGGL(k_crepe_viterbi, dim3((unsigned)n_clips), dim3(CV_THREADS), lds, c->stream, cr.doff.as<int64_t>(), cr.logp.as<double>(),
                           cr.tab.as<double>() + CR_BINS, c0, std::log(1.0 / CR_BINS + tiny), cr.ptr.as<unsigned short>(), cr.bins.as<int>());
    }
    {
        KernelTimer t(c, PCE_K_CREPE_DECODE);
        hipLaunchKernelGGL(k_crepe_gather, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, vit ? cr.bins.as<int>() : cr.amax.as<int>(),
                           cr.P.as<float>(), cr.tab.as<double>(), total, cr.f0.as<double>(), cr.per.as<float>());
    }
    PCE_HIP(c, hipGetLastError());
    return PCE_OK;
}

} // namespace

extern "C" {

int pce_crepe_load(pce_ctx *c, const pce_crepe_dims *dims, const float *weights, int64_t n_floats)
{
    if (!c || !dims || !weights) return PCE_E_INVALID;
    auto &cr = c->cr;
    int c_in[6], c_out[6];
    for (int i = 0; i < 6; i++) { c_out[i] = dims->c_out[i]; c_in[i] = i == 0 ? 1 : dims->c_out[i - 1]; }
    PCE_TRY(crepe_dims_ok(c, c_in, c_out));
    const int E = 4 * c_out[5];
    int64_t expect = (int64_t)CR_BINS * E + CR_BINS;
    for (int i = 0; i < 6; i++) expect += (int64_t)c_out[i] * (i == 0 ? CR_TAPS1 : CR_TAPS) * c_in[i] + 3 * (int64_t)c_out[i];
    if (n_floats != expect) return pce_fail(c, PCE_E_INVALID, "CREPE weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)expect);
    PCE_HIP(c, hipSetDevice(c->device));
    cr.loaded = false; cr.ran = false;
    DevBuf tmp;
    const float *w = weights;
    for (int i = 0; i < 6; i++) {
        const int64_t nw = (int64_t)c_out[i] * (i == 0 ? CR_TAPS1 : CR_TAPS) * c_in[i];
        PCE_TRY(upload_f16(c, w, nw, cr.w16[i], tmp));
        w += nw;
        PCE_UPLOAD(c, cr.bss[i], w, 3 * (size_t)c_out[i]);
        w += 3 * (int64_t)c_out[i];
    }
    PCE_UPLOAD(c, cr.cls_w, w, (size_t)CR_BINS * E);
    w += (int64_t)CR_BINS * E;
    PCE_UPLOAD(c, cr.cls_b, w, (size_t)CR_BINS);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 6; i++) { cr.c_in[i] = c_in[i]; cr.c_out[i] = c_out[i]; }
    cr.n_emb = E;
    cr.loaded = true;
    return PCE_OK;
}

int pce_crepe_run(pce_ctx *c, const pce_crepe_plan *plan)
{
    if (!c || !plan) return PCE_E_INVALID;
    auto &cr = c->cr;
    if (!cr.loaded) return pce_fail(c, PCE_E_STATE, "pce_crepe_run before pce_crepe_load");
    if (!c->d_pcm) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    if (c->rate != CR_RATE) return pce_fail(c, PCE_E_INVALID, "CREPE runs at 16000 Hz: the resident batch is at %d Hz (resample it first)", c->rate);
    if (plan->hop < 1 || plan->lo < 0 || plan->hi > CR_BINS || plan->lo >= plan->hi || (plan->decoder != 0 && plan->decoder != 1) || plan->frames_per_chunk < 1)
        return pce_fail(c, PCE_E_INVALID, "bad CREPE plan (hop >= 1, 0 <= lo < hi <= 360, decoder 0 | 1, frames_per_chunk >= 1)");
    PCE_HIP(c, hipSetDevice(c->device));
    cr.ran = false;
    cr.off.assign((size_t)c->n_clips + 1, 0);
    for (int32_t i = 0; i < c->n_clips; i++) {
        const int64_t len = c->clip_off[(size_t)i + 1] - c->clip_off[(size_t)i];
        cr.off[(size_t)i + 1] = cr.off[(size_t)i] + 1 + len / plan->hop;
    }
    const int64_t total = cr.off[(size_t)c->n_clips];
    if (c->n_clips == 0) { cr.ran = true; return PCE_OK; }
    // elements (fp16) of the images per frame; the chunk is clamped to the stated budget
    int64_t per_frame = CR_IMG1 + cr.n_emb;
    for (int i = 1; i < 6; i++) per_frame += crepe_img_elems(cr.c_in, i);
    int64_t F = plan->frames_per_chunk;
    if (F > total) F = total;
    const int64_t fit = PCE_CREPE_IMAGE_BUDGET / (per_frame * (int64_t)sizeof(h16));
    if (F > fit) F = fit;
    if (F < 1) F = 1;
    if (F > 32768) F = 32768;                                    // a launch's grid: one row tile (block 2) or one workgroup row (block 1) per frame
    const int E = cr.n_emb;
    for (int i = 0; i < 7; i++) {
        const int64_t elems = i == 0 ? CR_IMG1 : i == 6 ? E : crepe_img_elems(cr.c_in, i);
        PCE_ZERO(h16, c, cr.img[i], (size_t)(elems * F) + 32);                                             // the pad rows: once per run
    }
    PCE_TRY(crepe_decode_prepare(c, c->n_clips, total));
    const size_t cls_lds = sizeof(h16) * (size_t)CL_FRAMES * E;
    PCE_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_crepe_classifier), hipFuncAttributeMaxDynamicSharedMemorySize, (int)cls_lds));
    for (int64_t g0 = 0; g0 < total; g0 += F) {
        const int n = (int)(total - g0 < F ? total - g0 : F);
        {
            KernelTimer t(c, PCE_K_CREPE_FRAMES);
            hipLaunchKernelGGL(k_crepe_frames, dim3((unsigned)div_up(n, 4)), dim3(256), 0, c->stream, c->d_pcm, c->d_clip_off.as<int64_t>(),
                               cr.doff.as<int64_t>(), (int)c->n_clips, (int)plan->hop, g0, n, cr.img[0].as<h16>());
        }
        for (int b = 1; b <= 6; b++) {
            const bool last = b == 6;
            const int64_t ofs = last ? E : crepe_img_elems(cr.c_in, b);
            PCE_TRY(crepe_launch_block(c, b, cr.img[b - 1].as<h16>(), cr.c_in[b - 1], cr.c_out[b - 1], cr.w16[b - 1].as<h16>(), cr.bss[b - 1].as<float>(),
                                       cr.img[b].as<h16>(), ofs, last ? 0 : CR_PADL, n));
        }
        {
            KernelTimer t(c, PCE_K_CREPE_CLASSIFIER, nullptr, 2.0 * CR_BINS * (double)E * n);
            hipLaunchKernelGGL(k_crepe_classifier, dim3((unsigned)div_up(n, CL_FRAMES)), dim3(256), cls_lds, c->stream, cr.img[6].as<h16>(), E,
                               cr.cls_w.as<float>(), cr.cls_b.as<float>(), n, cr.P.as<float>() + g0 * CR_BINS);
        }
        PCE_HIP(c, hipGetLastError());
    }
    PCE_TRY(crepe_decode(c, c->n_clips, total, plan->lo, plan->hi, plan->decoder));
    PCE_HIP(c, hipGetLastError());
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    cr.decoder = plan->decoder;
    cr.ran = true;
    return PCE_OK;
}

int pce_crepe_shape(pce_ctx *c, int32_t clip, int64_t *n_frames)
{
    if (!c || !n_frames) return PCE_E_INVALID;
    if (!c->cr.ran) return pce_fail(c, PCE_E_STATE, "pce_crepe_shape before pce_crepe_run");
    if (clip < 0 || clip >= c->n_clips) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    *n_frames = c->cr.off[(size_t)clip + 1] - c->cr.off[(size_t)clip];
    return PCE_OK;
}

int pce_crepe_fetch(pce_ctx *c, int32_t clip, int32_t *bins, double *f0, float *periodicity, float *salience)
{
    if (!c) return PCE_E_INVALID;
    auto &cr = c->cr;
    if (!cr.ran) return pce_fail(c, PCE_E_STATE, "pce_crepe_fetch before pce_crepe_run");
    if (clip < 0 || clip >= c->n_clips) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    PCE_HIP(c, hipSetDevice(c->device));
    const int64_t g0 = cr.off[(size_t)clip], nf = cr.off[(size_t)clip + 1] - g0;
    const int *b = cr.decoder == 0 ? cr.bins.as<int>() : cr.amax.as<int>();
    if (bins) PCE_FETCH(c, bins, b + g0, (size_t)nf);
    if (f0) PCE_FETCH(c, f0, cr.f0.as<double>() + g0, (size_t)nf);
    if (periodicity) PCE_FETCH(c, periodicity, cr.per.as<float>() + g0, (size_t)nf);
    if (salience) PCE_FETCH(c, salience, cr.P.as<float>() + g0 * CR_BINS, (size_t)nf * CR_BINS);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

int pce_selftest_crepe_layer(pce_ctx *c, int32_t block, int32_t c_in, int32_t c_out, int32_t n_frames, const uint16_t *x, const uint16_t *w,
                             const float *bias, const float *scale, const float *shift, uint16_t *out)
{
    if (!c || !x || !w || !bias || !scale || !shift || !out) return PCE_E_INVALID;
    if (block < 1 || block > 6 || n_frames < 1 || n_frames > 32768) return pce_fail(c, PCE_E_INVALID, "block 1..6, 1 <= n_frames <= 32768");
    if (block == 1 ? (c_in != 1 || c_out % 64 != 0 || c_out < 64) : (c_in % 16 != 0 || c_in < 16 || c_out % 16 != 0 || c_out < 16) || c_in > 8192 || c_out > 8192)
        return pce_fail(c, PCE_E_LIMIT, "unsupported CREPE block widths");
    PCE_HIP(c, hipSetDevice(c->device));
    const int T = crepe_t_in(block), T_out = block == 1 ? 128 : T / 2;
    const int64_t in_row = block == 1 ? CR_IMG1 : (int64_t)(T + CR_PADL + CR_PADR) * c_in;
    const int64_t nw = (int64_t)c_out * (block == 1 ? CR_TAPS1 : CR_TAPS) * c_in, n_out = (int64_t)T_out * c_out;
    DevBuf d_in, d_w, d_bss, d_out;
    PCE_ZERO(h16, c, d_in, (size_t)(in_row * n_frames) + 32);
    PCE_HIP(c, d_out.reserve(sizeof(h16) * (size_t)(n_out * n_frames) + 64));
    const int64_t x_row = (int64_t)T * c_in, x_off = block == 1 ? CR_PAD1 : (int64_t)CR_PADL * c_in;
    PCE_HIP(c, hipMemcpy2DAsync(d_in.as<h16>() + x_off, sizeof(h16) * (size_t)in_row, x, sizeof(h16) * (size_t)x_row, sizeof(h16) * (size_t)x_row,
                                (size_t)n_frames, hipMemcpyHostToDevice, c->stream));
    PCE_UPLOAD(c, d_w, w, (size_t)nw, 32);
    PCE_UPLOAD(c, d_bss, bias, (size_t)c_out, 2 * (size_t)c_out);      // bias | scale | shift
    PCE_PUT(c, d_bss.as<float>() + c_out, scale, (size_t)c_out);
    PCE_PUT(c, d_bss.as<float>() + 2 * c_out, shift, (size_t)c_out);
    PCE_TRY(crepe_launch_block(c, block, d_in.as<h16>(), c_in, c_out, d_w.as<h16>(), d_bss.as<float>(), d_out.as<h16>(), n_out, 0, n_frames));
    PCE_HIP(c, hipGetLastError());
    PCE_FETCH(c, out, d_out.p, (size_t)(n_out * n_frames));
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

int pce_selftest_crepe_decode(pce_ctx *c, const float *salience, int32_t n_frames, int32_t lo, int32_t hi, int32_t decoder, int32_t *bins, double *f0,
                              float *periodicity)
{
    if (!c || !salience) return PCE_E_INVALID;
    if (n_frames < 1 || lo < 0 || hi > CR_BINS || lo >= hi || (decoder != 0 && decoder != 1)) return pce_fail(c, PCE_E_INVALID, "bad CREPE decode self-test arguments");
    auto &cr = c->cr;
    PCE_HIP(c, hipSetDevice(c->device));
    cr.ran = false;                                               // the results of the last pce_crepe_run are overwritten
    cr.off.assign({0, (int64_t)n_frames});
    PCE_TRY(crepe_decode_prepare(c, 1, n_frames));
    PCE_PUT(c, cr.P.p, salience, (size_t)n_frames * CR_BINS);
    PCE_TRY(crepe_decode(c, 1, n_frames, lo, hi, decoder));
    const int *b = decoder == 0 ? cr.bins.as<int>() : cr.amax.as<int>();
    if (bins) PCE_FETCH(c, bins, b, (size_t)n_frames);
    if (f0) PCE_FETCH(c, f0, cr.f0.p, (size_t)n_frames);
    if (periodicity) PCE_FETCH(c, periodicity, cr.per.p, (size_t)n_frames);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

} // extern "C"
