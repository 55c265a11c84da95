// pce_whisper_impl.inc -- the transformer work of the alignment step (R8) on gfx950: log-mel spectrogram, Whisper audio encoder,
// text decoder (teacher-forced forced alignment with cross-attention DTW; free-running greedy decoding with a K / V
// cache and openai-whisper's logit filters), and the break-prediction BERT forward, which shares the same kernels.
// This file: the kernels (with pce_gemm256.inc, pce_xattn.inc), WhisperState, the launchers, the log-mel and encoder entry points; it ends by
// including the other entry points: pce_whisper_selftest.inc, pce_whisper_decoder.inc, pce_bert.inc, pce_w2v.inc (one translation unit per operand type).
//
// Replaces the device work of whisper_timestamped.transcribe
// (Code/Aligners/use_whisper_timestamped.py:139,150-163), as openai-whisper==20240930 defines it (third-party,
// restated from its published architecture; the torch fp32 restatement in oracle/ is pinned against the installed
// transformers port of the same network: tests/test_whisper_hf_crosscheck.py):
//   log_mel_spectrogram: Hann(400) STFT hop 160 (centre, reflect padding), |.|^2, 80 Slaney
//     mel bands, log10(max(.,1e-10)), max(., max-8), (.+4)/4, 30 s window = 3000 frames
//   AudioEncoder: conv1d(80->d,k3,p1)+GELU, conv1d(d->d,k3,s2,p1)+GELU, + sinusoid positions,
//     L x { x += proj(MHA(LN(x)));  x += W2 gelu(W1 LN(x)) },  LN
//
// Execution plan:
//   k_logmel_frames  one wavefront per frame, 400-point DFT as 25 x 16 Cooley-Tukey in LDS (fp32),
//                    sparse mel bands, per-clip maximum by ordered-int atomicMax
//   k_logmel_norm    clamp/scale of the frames that hold audio into the op_t time-major padded image (the float [80][3000] matrix only on fetch)
//                    [3002][80] the first convolution reads as an implicit im2col GEMM operand
//   k_gemm_bf16      C = A B^T on v_mfma_f32_16x16x32_bf16: 128x128x64 tiles, 4 waves x (64x64),
//                    fp32 accumulate; operands stream global -> LDS with global_load_lds (16 B/lane),
//                    double buffered behind the MFMAs, XOR-swizzled chunks (conflict-free
//                    ds_read_b128), XCD-aware tile order, fused epilogues (bias, exact GELU,
//                    positional add, residual accumulate).
//                    Both convolutions are this GEMM with overlapping A rows (lda < K): the
//                    activations are time-major with zero pad rows, so "im2col" is just a stride.
//   k_layernorm      one wavefront per row, fp32 statistics
//   k_attention      flash-style forward per (clip, head, 64 queries): QK^T and PV on MFMA,
//                    online softmax in registers with DPP row reductions, K / V^T tiles in LDS
// The residual stream is fp32, every GEMM operand op_t.  Roofline: MFMA (dense op_t).
#include "pce_internal.h"
#include "pce_wave.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

// This file is compiled twice (pce_whisper_bf16.hip, pce_whisper_f16.hip): PCE_OP_T is the 16-bit operand type of every GEMM / attention
// product (fp32 accumulation and an fp32 residual stream in both builds), PCE_OP_INDEX the slot of the context that holds this build's
// state, PCE_WFN(name) the build's name for an entry point; pce_whisper_dispatch.hip exports the names of include/pce.h and forwards to
// the build the context selects (pce_whisper_set_operands).  bf16: the round-1 / round-2 arithmetic.  fp16: the reference's own --
// openai-whisper runs the model in half precision (fp16 activations and weights, fp32 LayerNorm and softmax; transcribe's fp16=True
// default behind Code/Aligners/use_whisper_timestamped.py:163): 11 significand bits instead of 8 at the same MFMA rate.
#define pce_logmel_run PCE_WFN(pce_logmel_run)
#define pce_logmel_run_at PCE_WFN(pce_logmel_run_at)
#define pce_logmel_fetch PCE_WFN(pce_logmel_fetch)
#define pce_selftest_logmel_image PCE_WFN(pce_selftest_logmel_image)
#define pce_whisper_load PCE_WFN(pce_whisper_load)
#define pce_whisper_encode_run PCE_WFN(pce_whisper_encode_run)
#define pce_whisper_encode_fetch PCE_WFN(pce_whisper_encode_fetch)
#define pce_selftest_attention PCE_WFN(pce_selftest_attention)
#define pce_selftest_attention_ragged PCE_WFN(pce_selftest_attention_ragged)
#define pce_selftest_attn1 PCE_WFN(pce_selftest_attn1)
#define pce_selftest_align_matrix PCE_WFN(pce_selftest_align_matrix)
#define pce_selftest_decode_rules PCE_WFN(pce_selftest_decode_rules)
#define pce_selftest_gemm PCE_WFN(pce_selftest_gemm)
#define pce_selftest_gemm_resid PCE_WFN(pce_selftest_gemm_resid)
#define pce_whisper_decoder_load PCE_WFN(pce_whisper_decoder_load)
#define pce_whisper_align_run PCE_WFN(pce_whisper_align_run)
#define pce_whisper_align_fetch PCE_WFN(pce_whisper_align_fetch)
#define pce_whisper_align_shape PCE_WFN(pce_whisper_align_shape)
#define pce_whisper_align_paths_enqueue PCE_WFN(pce_whisper_align_paths_enqueue)
#define pce_whisper_align_paths_wait PCE_WFN(pce_whisper_align_paths_wait)
#define pce_whisper_sample_keys PCE_WFN(pce_whisper_sample_keys)
#define pce_whisper_decode_step PCE_WFN(pce_whisper_decode_step)
#define pce_whisper_decode_step_ex PCE_WFN(pce_whisper_decode_step_ex)
#define pce_whisper_decode_loop PCE_WFN(pce_whisper_decode_loop)
#define pce_whisper_detect_language PCE_WFN(pce_whisper_detect_language)
#define pce_bert_load PCE_WFN(pce_bert_load)
#define pce_bert_run PCE_WFN(pce_bert_run)
#define pce_bert_fetch PCE_WFN(pce_bert_fetch)
#define pce_w2v_check PCE_WFN(pce_w2v_check)
#define pce_w2v_load PCE_WFN(pce_w2v_load)
#define pce_w2v_run PCE_WFN(pce_w2v_run)
#define pce_w2v_shape PCE_WFN(pce_w2v_shape)
#define pce_w2v_fetch PCE_WFN(pce_w2v_fetch)
#define pce_w2v_device PCE_WFN(pce_w2v_device)
#define pce_selftest_w2v_wave PCE_WFN(pce_selftest_w2v_wave)
#define pce_selftest_w2v_lngelu PCE_WFN(pce_selftest_w2v_lngelu)
#define pce_selftest_w2v_posconv PCE_WFN(pce_selftest_w2v_posconv)
#define pce_selftest_xattn PCE_WFN(pce_selftest_xattn)
#define pce_selftest_gemm_tiled PCE_WFN(pce_selftest_gemm_tiled)
#define pce_selftest_layernorm PCE_WFN(pce_selftest_layernorm)
#define pce_whisper_free PCE_WFN(pce_whisper_free)
extern "C" int pce_whisper_decode_step_ex(pce_ctx *c, const int32_t *tokens, const int32_t *token_offsets, const pce_whisper_decode_rules *rules,
                                          const uint8_t *vocab_mask, const pce_whisper_decode_opts *opts, int32_t *next_tokens,
                                          float *next_logprobs, float *probe_prob);
void pce_whisper_free(pce_ctx *c);

namespace {

typedef PCE_OP_T op_t;
typedef __attribute__((ext_vector_type(8))) op_t opx8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// the MFMA of this file's attention and GEMM kernels, on whichever 16-bit type the build computes in
template <class T> struct MfmaOf;
template <> struct MfmaOf<__bf16> {
    typedef __attribute__((ext_vector_type(8))) __bf16 v8;
    static __device__ __forceinline__ f32x4 m16(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct MfmaOf<_Float16> {
    typedef __attribute__((ext_vector_type(8))) _Float16 v8;
    static __device__ __forceinline__ f32x4 m16(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
__device__ __forceinline__ f32x4 mfma16(opx8 a, opx8 b, f32x4 c) { return MfmaOf<op_t>::m16(a, b, c); }

constexpr int W_NFFT = 400, W_HOP = 160, W_BINS = 201, W_FRAMES = 3000, W_SAMPLES = 480000;
constexpr int W_CTX = 1500;
// The conv stem does not multiply the rows of the zero padding behind a clip's audio (DESIGN.md section 5).  With P = the first padded frame of a
// clip's window (k_logmel_frames' predicate), frames P .. 2999 of the log-mel image are one constant row, so conv1 rows P+1 .. 2998 are one row
// and conv2 rows ceil((P+2)/2) .. 1498 have one accumulator row (row 1499 sees the zero row behind the window; the outputs differ by the
// positional row alone).  Conv2 runs its row tiles [0, s) and its last one, conv1 the tiles those read; k_stem_fill writes conv2 rows
// [ST_TILE s, ST_TILE ST_C2_LAST) from the accumulators of row ST_TILE ST_C2_LAST, which the last tile leaves behind.  s = ST_C2_LAST: nothing skipped.
constexpr int ST_TILE = 128;                                        // rows of a k_gemm_bf16 tile (G_BM)
constexpr int ST_C2_LAST = (W_CTX - 1) / ST_TILE;                   // conv2's last row tile (11): rows 1408 .. 1499, always computed
constexpr int ST_C1_KEEP = (2 * ST_TILE * ST_C2_LAST - 1) / ST_TILE; // first conv1 tile the last conv2 tile reads (21: frame 2815)
static_assert(ST_TILE * ST_C2_LAST < W_CTX - 1, "the last conv2 tile must hold a repeated row in front of row 1499");
struct GemmSkip {                   // k_gemm_bf16: row tiles tiles[z].x .. tiles[z].y of batch entry z return at once (tiles == nullptr: none);
    const int2 *tiles;              // rep != nullptr (EPI_GELU_POS_F32): the raw fp32 accumulators of row rep_row of every batch entry go to rep[z][N]
    float *rep; int rep_row;        // (rep_row % 128 == 0, in a tile no entry skips)
    int64_t skipped_rows;           // host side: the rows of all skipped tiles together, taken off the work count of the launch's timer
};
// The first conv2 row tile a clip leaves out (ST_C2_LAST: none), for a window that starts f_begin frames into len samples: P = the smallest f in
// [0, 3000] with (f_begin + f) * 160 - 200 >= len, the `padded` predicate of k_logmel_norm.  The device derives the ranges from it (k_logmel_norm), the
// host the batch's totals (logmel_run_impl): one expression for both.
__host__ __device__ inline int stem_first_skipped_tile(int64_t len, int64_t f_begin)
{
    const int64_t p64 = (len + W_NFFT / 2 + W_HOP - 1) / W_HOP - f_begin;
    const int P = (int)(p64 < 0 ? 0 : p64 > W_FRAMES ? W_FRAMES : p64);
    const int r2 = (P + 3) / 2;                                             // first conv2 row of the repeated accumulators, ceil((P + 2) / 2)
    const int s = (r2 + ST_TILE - 1) / ST_TILE;                             // conv2 tiles [s, ST_C2_LAST) hold nothing else
    return s < ST_C2_LAST ? s : ST_C2_LAST;
}
constexpr double W_PI = 3.14159265358979323846;

// ---------------------------------------------------------------------------
// log-mel
// ---------------------------------------------------------------------------
struct MelTables {            // device pointers
    const float2 *w16;        // [16]      exp(-2 pi i m / 16)
    const float2 *w400;       // [25][16]  exp(-2 pi i n2 k1 / 400)
    const float2 *w25;        // [25]      exp(-2 pi i m / 25)
    const float *window;      // [400]     periodic Hann
    const int *mel_lo;        // [n_mels]  first bin of band
    const int *mel_n;         // [n_mels]  number of bins
    const int *mel_off;       // [n_mels]  offset into mel_w
    const float *mel_w;       // packed weights
    int mel_total;            // number of packed weights (<= LM_MELW)
};

__device__ __forceinline__ unsigned int f32_order_key(float f)
{
    const unsigned int b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f32_from_key(unsigned int k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// frame0 == nullptr: the window is frames 0..2999 of the clip trimmed to 30 s (pad_or_trim + log_mel_spectrogram).
// frame0 != nullptr: whisper.transcribe's slicing of the log-mel of the WHOLE clip followed by 30 s of zeros: the window is
// frames frame0[clip] .. +2999, samples beyond 30 s exist, and (scan != 0) a first launch reduces the maximum over every
// frame that overlaps audio (the frames of pure padding are at the -10 floor) without writing anything.
constexpr int LM_MELW = 1024;             // packed mel weights k_logmel_frames keeps in LDS (80 bands: 404, 128 bands: 406)
// PCE_NO_PK_F32 (pce_internal.h): this kernel is compiled WITHOUT packed fp32 instructions.  The complex products below make the compiler
// form v_pk_mul_f32 / v_pk_add_f32 with op_sel:[0,1], and that selection returns wrong values in lanes 48..63 whenever another wave on the
// same SIMD executes MFMA -- the encoder of another process or of another stream (profiles/r06/multiprocess_glitch.txt: a frame of a clip's
// log-mel off now and then with three processes on one device; tools/lab/pk_victim.hip is the reduced case).  Same operations, same order, same bits.
template <int LM_G>                       // frames a wave processes before it writes their values (LM_G * 4 bytes per band and store)
__global__ __launch_bounds__(256) PCE_NO_PK_F32 void k_logmel_frames(const int16_t *__restrict__ pcm, const int64_t *__restrict__ clip_off, int n_mels,
                                                      MelTables T, float *__restrict__ logspec /* [clip][n_mels][3000] */,
                                                      unsigned int *__restrict__ clip_max, const int64_t *__restrict__ frame0, int scan)
{
    __shared__ float xs[4][W_NFFT];
    __shared__ float2 ys[4][25 * 16];
    __shared__ float pw[4][W_BINS + 3];
    __shared__ float2 s_w16[16], s_w25[25], s_w400[25 * 16];
    __shared__ float s_melw[LM_MELW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < T.mel_total; i += 256) s_melw[i] = T.mel_w[i];
    for (int i = tid; i < 16; i += 256) s_w16[i] = T.w16[i];
    for (int i = tid; i < 25; i += 256) s_w25[i] = T.w25[i];
    for (int i = tid; i < 400; i += 256) s_w400[i] = T.w400[i];
    __syncthreads();
    const int clip = blockIdx.y;
    const int64_t base = clip_off[clip], full = clip_off[clip + 1] - base;
    const int64_t len = frame0 ? full : min<int64_t>(full, (int64_t)W_SAMPLES);
    const int64_t f_begin = (frame0 && !scan) ? frame0[clip] : 0;
    const int64_t n_fr = scan ? (full + W_NFFT / 2) / W_HOP + 1 : W_FRAMES;       // scan: every frame that can see a sample
    // loop invariants of a lane (round 5: they were global loads inside the frame loop -- the band loop's were dependent ones, a latency chain of
    // up to 34 L2 round trips per frame): its seven window taps, the extent of its (up to two) mel bands
    float win[7];
#pragma unroll
    for (int i = 0; i < 7; i++) win[i] = (lane + 64 * i) < W_NFFT ? T.window[lane + 64 * i] : 0.f;
    int b_lo[2], b_cnt[2], b_off[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int b = lane + 64 * i;
        b_lo[i] = b < n_mels ? T.mel_lo[b] : 0; b_cnt[i] = b < n_mels ? T.mel_n[b] : 0; b_off[i] = b < n_mels ? T.mel_off[b] : 0;
    }
    float vmax = -1e30f;
    // A wave takes LM_G consecutive frames at a time and hands their log-mel values over through LDS, so that a band's row leaves as one
    // 64-byte segment per group (round 5: one 4-byte store per band and frame, 3 000 floats apart, was a read-modify-write of a sector each --
    // 4 x the kernel's algorithmic traffic in the PMC pass of round 4)
    extern __shared__ float lm_ob[];                              // [4 waves][n_mels][LM_G + 1]
    float *ob = lm_ob + (size_t)wv * n_mels * (LM_G + 1);
    const int64_t n_groups = (n_fr + LM_G - 1) / LM_G;
    for (int64_t gi = blockIdx.x * 4 + wv; gi < n_groups; gi += gridDim.x * 4) {
      for (int j = 0; j < LM_G; j++) {
        const int64_t fl = gi * LM_G + j;
        if (fl >= n_fr) break;
        const int64_t frame = f_begin + fl;
        if (frame * W_HOP - W_NFFT / 2 >= len) {
            // a frame of the zero padding behind the audio (two thirds of the 30 s window of a 10 s clip): every sample is an exact zero, so are
            // the spectrum and the mel energies, and the value is log10 of the 1e-10 clamp -- written without running the transform
            const float lg = log10f(fmaxf(0.f, 1e-10f));
            for (int b = lane; b < n_mels; b += 64) ob[b * (LM_G + 1) + j] = lg;
            vmax = fmaxf(vmax, lg);
            continue;
        }
        // windowed frame, centre = frame*160, reflect padding at the start, zeros past the audio
#pragma unroll
        for (int wi = 0; wi < 7; wi++) {
            const int n = lane + 64 * wi;
            if (n < W_NFFT) {
                int64_t i = frame * W_HOP - W_NFFT / 2 + n;
                if (i < 0) i = -i;
                const float v = (i < len) ? (float)pcm[base + i] * (1.0f / 32768.0f) : 0.0f;
                xs[wv][n] = v * win[wi];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
        // stage A: Y[n2][k1] = sum_{n1<16} x[25 n1 + n2] W16^{n1 k1}, then twiddle W400^{n2 k1}
        for (int o = lane; o < 400; o += 64) {
            const int n2 = o >> 4, k1 = o & 15;
            float re = 0.f, im = 0.f;
#pragma unroll
            for (int n1 = 0; n1 < 16; n1++) {
                const float x = xs[wv][25 * n1 + n2];
                const float2 w = s_w16[(n1 * k1) & 15];
                re = fmaf(x, w.x, re); im = fmaf(x, w.y, im);
            }
            const float2 t = s_w400[o];
            ys[wv][o] = make_float2(re * t.x - im * t.y, re * t.y + im * t.x);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
        // stage B: X[k1 + 16 k2] = sum_{n2<25} Y[n2][k1] W25^{n2 k2}; only k <= 200 is needed
        for (int k = lane; k < W_BINS; k += 64) {
            const int k1 = k & 15, k2 = k >> 4;
            float re = 0.f, im = 0.f;
            int m = 0;
            for (int n2 = 0; n2 < 25; n2++) {
                const float2 y = ys[wv][n2 * 16 + k1];
                const float2 w = s_w25[m];
                re += y.x * w.x - y.y * w.y; im += y.x * w.y + y.y * w.x;
                m += k2; if (m >= 25) m -= 25;
            }
            pw[wv][k] = re * re + im * im;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int bi = 0; bi < 2; bi++) {
            const int b = lane + 64 * bi;
            if (b < n_mels) {
                const int lo = b_lo[bi], cnt = b_cnt[bi];
                const float *w = s_melw + b_off[bi];
                float acc = 0.f;
                for (int i = 0; i < cnt; i++) acc = fmaf(w[i], pw[wv][lo + i], acc);
                const float lg = log10f(fmaxf(acc, 1e-10f));
                ob[b * (LM_G + 1) + j] = lg;
                vmax = fmaxf(vmax, lg);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      // (round 6) a group whose FIRST frame lies in the padding holds nothing but the clamp value: it is not written at all -- k_logmel_norm and the fetch
      // know the value (two thirds of the 30 s window of a 10 s clip: 163 of the 245 MB this kernel wrote per C3 step, and as many bytes the next pass read back)
      if (!scan && (f_begin + gi * LM_G) * W_HOP - W_NFFT / 2 < len) {
          const int64_t f0 = gi * LM_G;
          const int nj = (int)min<int64_t>(LM_G, n_fr - f0);
          for (int idx = lane; idx < n_mels * LM_G; idx += 64) {
              const int b = idx / LM_G, j = idx - b * LM_G;
              if (j < nj) logspec[((int64_t)clip * n_mels + b) * W_FRAMES + f0 + j] = ob[b * (LM_G + 1) + j];
          }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    }
    vmax = wave_xor_max(vmax);
    if (lane == 0) atomicMax(clip_max + clip, f32_order_key(vmax));
}

// max(x, max - 8), (x + 4) / 4 of clips clip0 .. clip0 + gridDim.z - 1 from the raw log10 values k_logmel_frames left ([clip][n_mels][3000]; frames of the padding
// are not stored: their value is the clamp constant) into what the CALLER consumes: out_tm = the op_t time-major padded image [clip][3002][n_mels] the conv stem
// reads (rows 0 and 3001 stay zero) -- pce_logmel_run; out_f32 = the float matrix [n_mels][3000] of ONE clip in a staging buffer -- pce_logmel_fetch.
// Round 5 rewrote the whole float matrix in place on every run (read 245 MB, write 245 + 123 MB per C3 step: 3.2 x the stage's algorithmic bytes); nothing on the
// device reads it.
__global__ __launch_bounds__(256) void k_logmel_norm(const float *__restrict__ logspec, const unsigned int *__restrict__ clip_max, int n_mels,
                                                    const int64_t *__restrict__ clip_off, const int64_t *__restrict__ frame0, int clip0,
                                                    op_t *__restrict__ out_tm, float *__restrict__ out_f32,
                                                    int2 *__restrict__ skip_c1, int2 *__restrict__ skip_c2)
{
    __shared__ float tile[64][65];
    const int clip = clip0 + blockIdx.z, f0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
    const float floor_v = f32_from_key(clip_max[clip]) - 8.0f;
    const int64_t full = clip_off[clip + 1] - clip_off[clip];
    const int64_t len = frame0 ? full : min<int64_t>(full, (int64_t)W_SAMPLES), f_begin = frame0 ? frame0[clip] : 0;
    if (skip_c1 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        // the row tiles the conv stem leaves out for this clip (ST_TILE above), from the image this launch writes
        const int s = stem_first_skipped_tile(len, f_begin);
        skip_c2[clip] = make_int2(s, ST_C2_LAST - 1);
        skip_c1[clip] = s < ST_C2_LAST ? make_int2(2 * s, ST_C1_KEEP - 1) : make_int2(1, 0);      // conv2 tiles [0, s) read conv1 rows < 2 ST_TILE s
    }
    const float pad_v = (fmaxf(log10f(fmaxf(0.f, 1e-10f)), floor_v) + 4.0f) / 4.0f;           // a frame of the zero padding (k_logmel_frames' own expression)
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const bool padded = (f_begin + f0 + tx) * W_HOP - W_NFFT / 2 >= len;
    for (int r = ty; r < 64; r += 4) {
        const int b = b0 + r, f = f0 + tx;
        if (b < n_mels && f < W_FRAMES) {
            const float v = padded ? pad_v : (fmaxf(logspec[((int64_t)clip * n_mels + b) * W_FRAMES + f], floor_v) + 4.0f) / 4.0f;
            if (out_f32) out_f32[(int64_t)b * W_FRAMES + f] = v;
            tile[r][tx] = v;
        }
    }
    if (!out_tm) return;
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int f = f0 + r, b = b0 + tx;
        if (b < n_mels && f < W_FRAMES) out_tm[((int64_t)clip * (W_FRAMES + 2) + f + 1) * n_mels + b] = (op_t)tile[tx][r];
    }
}

// ---------------------------------------------------------------------------
// GEMM  C[M x N] = A[M x K] * B[N x K]^T  (op_t in, fp32 accumulate)
// ---------------------------------------------------------------------------
enum { EPI_BF16 = 0, EPI_GELU_BF16 = 1, EPI_GELU_POS_F32 = 2, EPI_RESID_F32 = 3, EPI_QKV = 4, EPI_F32 = 5 };    // EPI_F32: C = A B^T + bias in fp32, C not read (the vocabulary logits)
constexpr int AT_SP = 1536;               // padded key axis of the transposed V image (multiple of the 64-key tile)
constexpr int G_BM = 128, G_BN = 128, G_BK = 64;
static_assert(G_BM == ST_TILE, "the stem's skip ranges count k_gemm_bf16 row tiles");

// GELU(x) = x/2 (1 + erf(x/sqrt 2)) = x/2 + |x|/2 erf(|x|/sqrt 2) (erf is odd: no sign select); erf by Abramowitz-Stegun 7.1.26,
// erf(z) = 1 - t P(t) exp(-z^2), t = 1/(1 + p z), |error| < 1.5e-7 -- far below the op_t step of the outputs (libm's erff costs more than
// the tile's MFMAs in a K = 768 epilogue).  With z' = z sqrt(log2 e) the exponential is a bare v_exp_f32 of -z'^2 and p z = (p / sqrt(log2 e)) z'.
// gelu_exact8 is the same operation sequence on eight values, written level by level: the eight dependency chains interleave, so the packed
// fp32 instructions the compiler forms need no wait states between them (the one-value form in a loop cost 18 issue slots per value, 4 of
// them s_nop; this costs 11).
constexpr float GELU_C = 0.70710678118654752440f * 1.2011224087864498f;     // |x| -> z' = |x| / sqrt 2 * sqrt(log2 e)
constexpr float GELU_P = 0.3275911f / 1.2011224087864498f;
__device__ __forceinline__ float gelu_exact(float x)
{
    const float zp = fabsf(x) * GELU_C;
    const float t = __builtin_amdgcn_rcpf(fmaf(zp, GELU_P, 1.0f));         // v_rcp_f32 (1 ulp); __frcp_rn expands to a 10-instruction IEEE division
    const float e = __builtin_amdgcn_exp2f(zp * -zp);
    const float poly = fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
    const float erf_abs = fmaf(-(t * poly), e, 1.0f);
    const float h = 0.5f * x;
    return fmaf(fabsf(h), erf_abs, h);
}
__device__ __forceinline__ void gelu_exact8(float (&x)[8])
{
    float zp[8], t[8], e[8], poly[8], h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) zp[i] = fabsf(x[i]) * GELU_C;
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = __builtin_amdgcn_rcpf(fmaf(zp[i], GELU_P, 1.0f));
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = __builtin_amdgcn_exp2f(zp[i] * -zp[i]);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = fmaf(t[i], 1.061405429f, -1.453152027f);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = fmaf(t[i], poly[i], 1.421413741f);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = fmaf(t[i], poly[i], -0.284496736f);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = fmaf(t[i], poly[i], 0.254829592f);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = t[i] * poly[i];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = fmaf(-poly[i], e[i], 1.0f);
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = 0.5f * x[i];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = fmaf(fabsf(h[i]), e[i], h[i]);
}

// LDS image of one operand tile: 128 rows x 64 op_t (128 B = eight 16-byte chunks per row), rows
// contiguous (what global_load_lds writes: wave-uniform base + lane * 16 B).  To keep the fragment
// reads (16 rows x one chunk per ds_read_b128 lane group) conflict-free the chunk index is
// XOR-swizzled with (row >> 1) & 7: applied to the GLOBAL source address when staging and to the
// LDS address when reading (the same involution on both sides).
__device__ __forceinline__ int swz_chunk(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

constexpr int G_THREADS = 512;
constexpr int G_TLD = G_BN + 4;           // fp32 epilogue tile row (pad keeps the accumulator scatter conflict-free)

// one operand tile (128 rows x 64 k): 16 wave-instructions of 1 KiB (8 rows each); 8 waves -> 2 each
__device__ __forceinline__ void stage_tile(const op_t *__restrict__ G, int64_t ld, int row0, int row_max, int k0, op_t *lds_tile, int wv, int lane)
{
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int r0 = wv * 16 + i * 8;
        const int row = r0 + (lane >> 3);
        const int c = swz_chunk(row, lane & 7);
        int gr = row0 + row; if (gr > row_max) gr = row_max;
        const op_t *src = G + (int64_t)gr * ld + k0 + c * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(lds_tile + r0 * G_BK), 16, 0, 0);
    }
}

template <int EPI>
__device__ __forceinline__ void gemm_fetch_bias(const float *__restrict__ bias, int n0, int tid, float (&bv)[8], float &bv_col)
{
    constexpr bool OUT_BF16 = (EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_QKV);
    const int cx0 = OUT_BF16 ? (tid & 15) * 8 : (tid & 31) * 4;
#pragma unroll
    for (int e = 0; e < 8; e++) bv[e] = (bias && e < (OUT_BF16 ? 8 : 4)) ? bias[n0 + cx0 + e] : 0.f;
    bv_col = (EPI == EPI_QKV && bias) ? bias[n0 + (tid & 127)] : 0.f;      // transposed-V path: one column per thread
}

// Output stage shared by the GEMM kernels: a [128][G_TLD] fp32 tile in LDS (rows m0.., columns n0..) leaves as full
// 256-byte row segments with the fused bias / GELU / positional add / residual accumulate / transposed-V write.
// bv / bv_col: this thread's bias values for the tile's columns, fetched by the caller before its K loop.
template <int EPI>
__device__ __forceinline__ void gemm_store_tile(const float *tile, int tid, int m0, int n0, int M, int N, const float (&bv)[8], float bv_col,
                                                void *__restrict__ Cv, int64_t ldc, int64_t cbase, const float *__restrict__ pos, int pos_T,
                                                int v_col0, int vt_sp, float *__restrict__ rep = nullptr, int rep_row = 0)
{
    if (EPI == EPI_QKV && n0 >= v_col0) {
        // V columns: written transposed, vt[clip][head][d][key], so the attention kernel can stage V^T tiles
        // (8 keys contiguous per d) without an LDS transpose.  `pos` carries the vt pointer, pos_T = S.
        op_t *vt = reinterpret_cast<op_t *>(const_cast<float *>(pos));
        const int dmodel = N - v_col0, S = pos_T;                   // V is the last d_model columns
        const int cc = tid & 127, rg = tid >> 7;                  // one column, 8-row groups
        const int n = n0 + cc - v_col0, head = n >> 6, dd = n & 63;
        const float bv = bv_col;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = rg * 8 + 32 * p;
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {                      // halves of 4 tokens never straddle a clip (S % 4 == 0)
                const int m = m0 + row + 4 * hf;
                if (m >= M) continue;
                const int clip = m / S, t = m - clip * S;
                typedef __attribute__((ext_vector_type(4))) op_t opx4;
                opx4 o;
#pragma unroll
                for (int e = 0; e < 4; e++) o[e] = (op_t)(tile[(row + 4 * hf + e) * G_TLD + cc] + bv);
                *reinterpret_cast<opx4 *>(vt + (((int64_t)clip * (dmodel >> 6) + head) * 64 + dd) * vt_sp + t) = o;
            }
        }
    } else if (EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_QKV) {
        // 16 threads x 8 columns per row, 32 rows per pass
        const int cx = (tid & 15) * 8, ry = tid >> 4;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = ry + 32 * p;
            if (m0 + row >= M) continue;
            const float4 v0 = *reinterpret_cast<const float4 *>(&tile[row * G_TLD + cx]);
            const float4 v1 = *reinterpret_cast<const float4 *>(&tile[row * G_TLD + cx + 4]);
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            opx8 o;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float t = v[e] + bv[e];
                o[e] = (op_t)(EPI == EPI_GELU_BF16 ? gelu_exact(t) : t);
            }
            // written once, read by the next kernel: keep it out of the way of the operand tiles in L2
            __builtin_nontemporal_store(o, reinterpret_cast<opx8 *>(reinterpret_cast<op_t *>(Cv) + cbase + (int64_t)(m0 + row) * ldc + n0 + cx));
        }
    } else {
        // fp32 outputs: 32 threads x 4 columns per row, 16 rows per pass
        const int cx = (tid & 31) * 4, ry = tid >> 5;
        float4 oldv[8];
        if (EPI == EPI_RESID_F32) {
#pragma unroll
            for (int p = 0; p < 8; p++) {                         // all eight residual loads in flight together
                const int row = ry + 16 * p;
                oldv[p] = m0 + row < M ? *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(Cv) + cbase + (int64_t)(m0 + row) * ldc + n0 + cx)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int p = 0; p < 8; p++) {
            const int row = ry + 16 * p;
            if (m0 + row >= M) continue;
            const float4 v = *reinterpret_cast<const float4 *>(&tile[row * G_TLD + cx]);
            float4 *dst = reinterpret_cast<float4 *>(reinterpret_cast<float *>(Cv) + cbase + (int64_t)(m0 + row) * ldc + n0 + cx);
            float4 o;
            if (EPI == EPI_GELU_POS_F32) {
                // (conv2 of the stem) the accumulators of the row whose output the skipped rows repeat: k_stem_fill finishes them with the expression below
                if (rep && m0 + row == rep_row) *reinterpret_cast<float4 *>(rep + n0 + cx) = v;
                const float4 pe = *reinterpret_cast<const float4 *>(pos + (int64_t)((m0 + row) % pos_T) * N + n0 + cx);
                o = make_float4(gelu_exact(v.x + bv[0]) + pe.x, gelu_exact(v.y + bv[1]) + pe.y, gelu_exact(v.z + bv[2]) + pe.z,
                                gelu_exact(v.w + bv[3]) + pe.w);
            } else {
                const float4 old = EPI == EPI_RESID_F32 ? oldv[p] : make_float4(0.f, 0.f, 0.f, 0.f);      // (0 + v is v: the bits of the former cleared-C form)
                o = make_float4(old.x + v.x + bv[0], old.y + v.y + bv[1], old.z + v.z + bv[2], old.w + v.w + bv[3]);
            }
            *dst = o;
        }
    }
}

// 8 wavefronts as 2 (M) x 4 (N), each owning a 64 x 32 slice of the 128 x 128 tile.  Three LDS stages:
// while tile kt is multiplied, tiles kt+1 and kt+2 are in flight as LDS-DMA (4 instructions per wave and
// tile), so a tile has two full K-steps to arrive.  The barrier is a raw s_barrier behind a COUNTED
// s_waitcnt vmcnt(4): __syncthreads() would drain the DMA queue (vmcnt(0)) and serialise the ring.
// G_STAGES = 2: two workgroups per CU cover each other's waits (big grids).  G_STAGES = 4 (round 3): the few-row launches of an
// incremental decoding step (M = clips: 2 x N/128 workgroups on 256 CUs) are alone on their CU and each K-step waited out a full
// L2 / HBM round trip (12 K-steps x 1.5 us = the 24 us such a launch took); with three tiles in flight the K loop runs at the
// DMA issue rate instead.
template <int EPI, int G_STAGES = 2>
__global__ __launch_bounds__(G_THREADS, G_STAGES == 2 ? 4 : 2) void k_gemm_bf16(const op_t *__restrict__ A, int64_t lda, int64_t a_batch,
                                                        const op_t *__restrict__ B, int M, int N, int K,
                                                        const float *__restrict__ bias, void *__restrict__ Cv, int64_t ldc, int64_t c_batch,
                                                        const float *__restrict__ pos, int pos_T, int v_col0, int vt_sp, int sn_tiles, int sm_tiles,
                                                        GemmSkip skip)
{
    // operand ring [stage][A|B][128][64] op_t, re-used as the fp32 epilogue tile [128][G_TLD]
    constexpr int SMEM_ELEMS = (G_STAGES * 2 * G_BM * G_BK * 2 > G_BM * G_TLD * 4 ? G_STAGES * 2 * G_BM * G_BK : G_BM * G_TLD * 2);
    __shared__ __attribute__((aligned(1024))) op_t smem[SMEM_ELEMS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = wv >> 2, wc = wv & 3;
    // XCD-aware, L2-sized tile order.  Workgroups go to the 8 XCDs round-robin, so XCD x is given a contiguous range of
    // the tile sequence, and the ~64 workgroups resident on an XCD at a time are 64 consecutive tiles of it.  The
    // sequence walks SUPERTILES of sm (M) x sn (N) tiles: their operands (sm A row blocks + sn B row blocks of 128 x K)
    // fit the XCD's 4 MB L2 and every block is re-read 8 times from it.  (A plain row-major sequence keeps 2-3 A blocks
    // and ALL of B live: at N = 3072 that is 4.7 MB of weights, which evicts itself; measured L2 hit rate 50 %.)
    const int tiles_n = (int)gridDim.x, tiles_m_pad = (int)gridDim.y;          // gridDim.y is padded to a multiple of 8
    int lin = (int)blockIdx.y * tiles_n + (int)blockIdx.x;
    const int total = tiles_n * tiles_m_pad;
    // With a skip description the XCD's range rotates with the batch entry: every entry skips the SAME stretch of the sequence (a 10 s clip: conv2's row
    // tiles 4-10 beside the grid's padding tiles 12-15), and un-rotated the XCDs that own that stretch idle through the whole launch while two of them carry
    // all the work (measured: 58 % of the tiles skipped, 6 % of the time).  Which workgroup computes a tile does not change the tile.
    if ((total & 7) == 0) lin = (((lin & 7) + (skip.tiles ? (int)blockIdx.z : 0)) & 7) * (total >> 3) + (lin >> 3);
    int m0, n0;
    {
        const int per = sm_tiles * sn_tiles, sup = lin / per, r = lin - sup * per;
        const int n_sn = tiles_n / sn_tiles;
        const int tm = (sup / n_sn) * sm_tiles + r / sn_tiles, tn = (sup % n_sn) * sn_tiles + r % sn_tiles;
        m0 = tm * G_BM; n0 = tn * G_BN;
        if (m0 >= M) return;                                                     // padding tile
        if (skip.tiles) {                                                        // a tile this batch entry does not need (the conv stem: rows of the zero padding)
            const int2 sk = skip.tiles[blockIdx.z];
            if (tm >= sk.x && tm <= sk.y) return;
        }
    }
    // the epilogue's bias values are fetched now: after the K loop their load latency (1-2 us) was fully exposed
    float bv[8]; float bv_col;
    gemm_fetch_bias<EPI>(bias, n0, tid, bv, bv_col);
    A += (int64_t)blockIdx.z * a_batch;
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    const int nk = K / G_BK;
    constexpr int STAGE = 2 * G_BM * G_BK;
    // prologue: tiles 0 .. G_STAGES - 2 (every tile is 4 DMA instructions per wave; a tile past the end of K is issued anyway -- the last
    // tile again, into a slot nobody reads -- so that the counted waits below are the same in every iteration)
#pragma unroll
    for (int t = 0; t < G_STAGES - 1; t++) {
        const int tt = t < nk ? t : nk - 1;
        stage_tile(A, lda, m0, M - 1, tt * G_BK, smem + t * STAGE, wv, lane);
        stage_tile(B, K, n0, N - 1, tt * G_BK, smem + t * STAGE + G_BM * G_BK, wv, lane);
    }
    for (int kt = 0; kt < nk; kt++) {
        const op_t *sA = smem + (kt % G_STAGES) * STAGE, *sB = sA + G_BM * G_BK;
        // tile kt has landed once at most the DMAs of the G_STAGES - 2 younger tiles of this wave are outstanding
        __builtin_amdgcn_s_waitcnt(0x0F70 | (((4 * (G_STAGES - 2)) >> 4) << 14) | ((4 * (G_STAGES - 2)) & 15));
        __builtin_amdgcn_s_barrier();
        if (G_STAGES > 2 || kt + G_STAGES - 1 < nk) {        // refill the stage tile kt-1 has just released (deep ring: always, see the prologue)
            const int tn = kt + G_STAGES - 1 < nk ? kt + G_STAGES - 1 : nk - 1;
            op_t *nA = smem + ((kt + G_STAGES - 1) % G_STAGES) * STAGE;
            stage_tile(A, lda, m0, M - 1, tn * G_BK, nA, wv, lane);
            stage_tile(B, K, n0, N - 1, tn * G_BK, nA + G_BM * G_BK, wv, lane);
        }
#pragma unroll
        for (int kk = 0; kk < G_BK; kk += 32) {
            opx8 a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = wr * 64 + i * 16 + fr;
                a[i] = *reinterpret_cast<const opx8 *>(&sA[row * G_BK + swz_chunk(row, (kk >> 3) + fq) * 8]);
            }
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int row = wc * 32 + j * 16 + fr;
                b[j] = *reinterpret_cast<const opx8 *>(&sB[row * G_BK + swz_chunk(row, (kk >> 3) + fq) * 8]);
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
        }
    }
    // epilogue.  The accumulator layout (col = lane & 15, row = (lane >> 4) * 4 + reg) would store 2-byte
    // elements 32 B at a time; measured, such an epilogue cost more than the whole K loop.  The tile
    // goes through LDS instead (the operand ring is free now) and leaves as full 256-B row segments.
    if (G_STAGES > 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the surplus refills of the deep ring must have landed before the ring is reused
    __builtin_amdgcn_s_barrier();                           // every wave is done reading the operand stages
    float *tile = reinterpret_cast<float *>(smem);           // [128][G_TLD] fp32 = 66 KiB
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                tile[(wr * 64 + i * 16 + fq * 4 + r) * G_TLD + wc * 32 + j * 16 + fr] = acc[i][j][r];
    __syncthreads();
    gemm_store_tile<EPI>(tile, tid, m0, n0, M, N, bv, bv_col, Cv, ldc, (int64_t)blockIdx.z * c_batch, pos, pos_T, v_col0, vt_sp,
                         skip.rep ? skip.rep + (int64_t)blockIdx.z * N : nullptr, skip.rep_row);
}

// k_stem_fill: the conv2 rows k_gemm_bf16 skipped (GemmSkip).  Rows [ST_TILE s, ST_TILE ST_C2_LAST) of clip blockIdx.y, s = tiles[clip].x, have the
// accumulators of the row the last tile left in rep[clip][d]; what differs is the positional row.  The expression is EPI_GELU_POS_F32's, so the bits are.
constexpr int SF_ROWS = 16;                                   // rows per workgroup (divides ST_TILE: a workgroup is skipped rows only, or none)
static_assert(ST_TILE % SF_ROWS == 0, "a fill workgroup must not straddle a tile boundary");
__global__ __launch_bounds__(256) void k_stem_fill(const int2 *__restrict__ tiles, const float *__restrict__ rep, const float *__restrict__ bias,
                                                   const float *__restrict__ pos /* [W_CTX][d] */, int d /* % 4 == 0 */, float *__restrict__ out /* [clip][W_CTX][d] */)
{
    const int clip = blockIdx.y, t0 = blockIdx.x * SF_ROWS;
    if (t0 < tiles[clip].x * ST_TILE || t0 >= ST_C2_LAST * ST_TILE) return;
    const int d4 = d >> 2;
    const float *acc = rep + (int64_t)clip * d;
    float *dst = out + ((int64_t)clip * W_CTX + t0) * d;
    const float *pe0 = pos + (int64_t)t0 * d;
    for (int i = threadIdx.x; i < SF_ROWS * d4; i += 256) {
        const int cx = (i % d4) * 4;
        const float4 v = *reinterpret_cast<const float4 *>(acc + cx), b = *reinterpret_cast<const float4 *>(bias + cx);
        const float4 pe = *reinterpret_cast<const float4 *>(pe0 + (int64_t)i * 4);
        const float4 o = make_float4(gelu_exact(v.x + b.x) + pe.x, gelu_exact(v.y + b.y) + pe.y, gelu_exact(v.z + b.z) + pe.z, gelu_exact(v.w + b.w) + pe.w);
        *reinterpret_cast<float4 *>(dst + (int64_t)i * 4) = o;
    }
}

// ---------------------------------------------------------------------------
// k_gemm_skinny (round 3): the projections of an incremental decoding step, C[M][N] with M = the number of sequences (a few hundred rows)
// and N, K <= a few thousand.  Such a launch is a LATENCY chain, not a throughput problem: the 128 x 128 kernel puts 2 x N/128
// workgroups on 256 CUs and each walks K in 64-deep steps (10-26 us per launch, 74 launches per decoding step).  Here a workgroup
// owns 64 rows x 32 columns (M/64 x N/32 workgroups: 96 for a 768-wide projection of 256 rows) and streams K in 256-deep chunks
// through three LDS buffers (48 KB each: 64 + 32 rows of 512 B), two chunks ahead: a K = 768 product has ALL its operand bytes in
// flight before the first MFMA (one memory round trip), K = 3072 keeps 96 KB per CU in flight.  4 waves, 16 rows x 32 columns
// each, accumulators stored straight from registers (a tile is 8 KB: no LDS pass).
// ---------------------------------------------------------------------------
constexpr int S_BM = 64, S_BN = 32, S_KC = 256, S_THREADS = 256, S_NBUF = 3;
constexpr int S_BUF = (S_BM + S_BN) * S_KC;                       // elements per buffer (48 KB)
constexpr int S_LDS = S_NBUF * S_BUF * 2;                          // dynamic LDS of a launch (bytes)
__device__ __forceinline__ int swz512(int row, int chunk) { return chunk ^ (row & 15); }     // 512-byte rows: 32 chunks, the low four bits swizzled
template <int EPI>
__global__ __launch_bounds__(S_THREADS) void k_gemm_skinny(const op_t *__restrict__ A, int64_t lda, const op_t *__restrict__ B, int M, int N, int K,
                                                           const float *__restrict__ bias, void *__restrict__ Cv, int64_t ldc)
{
    extern __shared__ __attribute__((aligned(1024))) op_t sk[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.x * S_BN, m0 = blockIdx.y * S_BM;
    const int nk = K / S_KC;
    // one chunk = 96 rows of 512 B = 48 wave-instructions of 2 rows; wave w issues instructions w, w + 4, ... (12 each)
    auto stage = [&](int kc, int buf) {
        op_t *dst = sk + buf * S_BUF;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const int inst = wv + 4 * i, row = inst * 2 + (lane >> 5);               // LDS row 0..95: 0..63 = A, 64..95 = B
            const int c = swz512(row, lane & 31);
            const op_t *src;
            if (row < S_BM) { int gr = m0 + row; if (gr > M - 1) gr = M - 1; src = A + (int64_t)gr * lda + kc * S_KC + c * 8; }
            else { int gr = n0 + row - S_BM; if (gr > N - 1) gr = N - 1; src = B + (int64_t)gr * K + kc * S_KC + c * 8; }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(dst + inst * 2 * S_KC), 16, 0, 0);
        }
    };
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    // The products are formed TRANSPOSED (weights as the A operand, activations as B: D[column][row]), so a lane ends up with four CONSECUTIVE
    // columns 4 fq .. 4 fq + 3 of ONE row (wave row fr) per 16-column block: the tile leaves as 8- / 16-byte stores (and the old residual values
    // arrive as 16-byte loads) instead of four 2- / 4-byte ones per block -- the same sums in the same order, the same bits.
    // the epilogue's bias values now: their latency hides behind the operand stream (the counted waits below retire them first)
    const int e_row = m0 + wv * 16 + fr;
    f32x4 bvec[2];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) { const int col = n0 + j * 16 + fq * 4 + r; bvec[j][r] = (bias && col < N) ? bias[col] : 0.f; }
    // ... and, for the accumulate-into-the-residual epilogue, the old values of C (round 5: fetched after the K loop they were a second,
    // fully exposed memory round trip of every out-projection / fc2 launch)
    f32x4 old_c[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (EPI == EPI_RESID_F32) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int col = n0 + j * 16 + fq * 4;
            if (e_row < M && col + 3 < N) old_c[j] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(Cv) + (int64_t)e_row * ldc + col);
            else if (e_row < M)
#pragma unroll
                for (int r = 0; r < 4; r++) if (col + r < N) old_c[j][r] = reinterpret_cast<const float *>(Cv)[(int64_t)e_row * ldc + col + r];
        }
    }
    // K <= 3 chunks (every projection of a decoding step but fc2): the whole product is in flight before the first MFMA -- ONE memory round
    // trip; longer K keeps two chunks ahead.  (A chunk past the end is issued anyway, into a buffer nobody reads, so that the counted waits
    // are the same in every iteration.)
    const bool all_up_front = nk <= S_NBUF;
#pragma unroll
    for (int t = 0; t < S_NBUF - 1; t++) stage(t < nk ? t : nk - 1, t);
    if (all_up_front) stage(nk - 1, S_NBUF - 1);                 // chunk 2 of a three-chunk product (a shorter one: its last chunk again, unread)
    for (int kc = 0; kc < nk; kc++) {
        // chunk kc has landed once at most the DMA instructions of the younger chunks are outstanding in this wave
        if (all_up_front) {
            if (kc == 0) __builtin_amdgcn_s_waitcnt(0x0F70 | (((24) >> 4) << 14) | ((24) & 15));
            else if (kc == 1) __builtin_amdgcn_s_waitcnt(0x0F70 | 12);
            else __builtin_amdgcn_s_waitcnt(0x0F70 | 0);
            __builtin_amdgcn_s_barrier();
        } else {
            __builtin_amdgcn_s_waitcnt(0x0F70 | 12);
            __builtin_amdgcn_s_barrier();
            const int tn = kc + S_NBUF - 1; stage(tn < nk ? tn : nk - 1, tn % S_NBUF);
        }
        const op_t *sA = sk + (kc % S_NBUF) * S_BUF, *sB = sA + S_BM * S_KC;
#pragma unroll
        for (int ks = 0; ks < S_KC / 32; ks++) {
            const int ra = wv * 16 + fr;
            const opx8 a = *reinterpret_cast<const opx8 *>(&sA[ra * S_KC + swz512(ra, ks * 4 + fq) * 8]);
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int rb = j * 16 + fr;                                       // (LDS row 64 + rb: (64 + rb) & 15 == rb & 15)
                const opx8 b = *reinterpret_cast<const opx8 *>(&sB[rb * S_KC + swz512(rb, ks * 4 + fq) * 8]);
                acc[j] = mfma16(b, a, acc[j]);                                    // (transposed: see above)
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the surplus refills land before the wave (and its LDS allocation) ends
    // D layout of the transposed 16 x 16 product: activation row = lane & 15, columns (lane >> 4) * 4 + register
    if (e_row >= M) return;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int col = n0 + j * 16 + fq * 4;
        float t[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // (the same association as the tiled kernels' epilogues -- (old + sum) + bias -- so that a row's bits do not depend on which kernel its batch size selects)
            if (EPI == EPI_RESID_F32) t[r] = (old_c[j][r] + acc[j][r]) + bvec[j][r];
            else { const float v = acc[j][r] + bvec[j][r]; t[r] = EPI == EPI_GELU_BF16 ? gelu_exact(v) : v; }
        }
        if (col + 3 < N) {
            if (EPI == EPI_RESID_F32) *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(Cv) + (int64_t)e_row * ldc + col) = f32x4{t[0], t[1], t[2], t[3]};
            else {
                typedef __attribute__((ext_vector_type(4))) op_t opx4;
                *reinterpret_cast<opx4 *>(reinterpret_cast<op_t *>(Cv) + (int64_t)e_row * ldc + col) = opx4{(op_t)t[0], (op_t)t[1], (op_t)t[2], (op_t)t[3]};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (col + r < N) {
                    if (EPI == EPI_RESID_F32) reinterpret_cast<float *>(Cv)[(int64_t)e_row * ldc + col + r] = t[r];
                    else reinterpret_cast<op_t *>(Cv)[(int64_t)e_row * ldc + col + r] = (op_t)t[r];
                }
        }
    }
}

// ---------------------------------------------------------------------------
// 128 x 256 tile variant for wide outputs (N >= 2048: QKV, fc1).  Skipping the A-operand loads of the 128 x 128 kernel
// speeds the encoder up by 36 %, skipping the B loads by 12 % (ablation): the ACTIVATION stream is what these launches
// wait for.  A tile twice as wide reads every A row block half as often; the weights (B) stay L2-resident anyway.
// 8 waves as 2 (M) x 4 (N), 64 x 64 per wave, 32-deep K-steps (16 MFMAs per wave between barriers, as before), two
// 24 KB stages so that two workgroups still share a CU, and the output leaves through the same 128 x 128 LDS tile
// in two column passes.
// ---------------------------------------------------------------------------
constexpr int W_BN = 256, W_BK = 32, W_STAGES = 2;   // a third stage (72 KB, still two workgroups per CU) measured +0.2 %: not latency bound
constexpr int W_STAGE = (G_BM + W_BN) * W_BK;                   // op_t elements per stage (24 KB)
// 64-byte rows (see swz_chunk).  A ds_read_b128 is serviced in four groups of sixteen lanes that are NOT lane-contiguous ({0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31}, ...: MI355X_MICROARCH.md, LDS): a fragment read (lane = 16 k-chunk + row) puts rows 0-3 and 12-15 of one chunk and
// rows 4-11 of the next into one group.  chunk ^ (row >> 2) left them two to a bank (SQ_LDS_BANK_CONFLICT 44 % of the LDS cycles of
// k_gemm_wide); chunk ^ (-(row >> 2) & 3) gives every lane of a group its own 16 bytes of the 256-byte bank row.
__device__ __forceinline__ int swz32(int row, int chunk) { return chunk ^ ((-(row >> 2)) & 3); }
// ROWS x 32 k operand tile: wave-instructions of 1 KiB (16 rows each)
template <int ROWS>
__device__ __forceinline__ void stage_rows32(const op_t *__restrict__ G, int64_t ld, int row0, int row_max, int k0, op_t *lds_tile, int wv, int lane)
{
#pragma unroll
    for (int i = 0; i < ROWS / 128; i++) {
        const int r0 = (wv + 8 * i) * 16;
        const int row = r0 + (lane >> 2);
        const int c = swz32(row, lane & 3);
        int gr = row0 + row; if (gr > row_max) gr = row_max;
        const op_t *src = G + (int64_t)gr * ld + k0 + c * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(lds_tile + r0 * W_BK), 16, 0, 0);
    }
}

template <int EPI>
__global__ __launch_bounds__(G_THREADS, 4) void k_gemm_wide(const op_t *__restrict__ A, int64_t lda, int64_t a_batch,
                                                        const op_t *__restrict__ B, int M, int N, int K,
                                                        const float *__restrict__ bias, void *__restrict__ Cv, int64_t ldc, int64_t c_batch,
                                                        const float *__restrict__ pos, int pos_T, int v_col0, int vt_sp, int sn_tiles, int sm_tiles)
{
    constexpr int SMEM_ELEMS = (W_STAGES * W_STAGE * 2 > G_BM * G_TLD * 4 ? W_STAGES * W_STAGE : G_BM * G_TLD * 2);
    __shared__ __attribute__((aligned(1024))) op_t smem[SMEM_ELEMS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = wv >> 2, wc = wv & 3;                         // 2 x 4 waves, 64 x 64 each
    const int tiles_n = (int)gridDim.x, tiles_m_pad = (int)gridDim.y;
    int lin = (int)blockIdx.y * tiles_n + (int)blockIdx.x;
    const int total = tiles_n * tiles_m_pad;
    if ((total & 7) == 0) lin = (lin & 7) * (total >> 3) + (lin >> 3);
    int m0, n0;
    {
        const int per = sm_tiles * sn_tiles, sup = lin / per, r = lin - sup * per;
        const int n_sn = tiles_n / sn_tiles;
        const int tm = (sup / n_sn) * sm_tiles + r / sn_tiles, tn = (sup % n_sn) * sn_tiles + r % sn_tiles;
        m0 = tm * G_BM; n0 = tn * W_BN;
        if (m0 >= M) return;
    }
    float bv0[8], bv1[8]; float bc0, bc1;
    gemm_fetch_bias<EPI>(bias, n0, tid, bv0, bc0);
    gemm_fetch_bias<EPI>(bias, n0 + 128, tid, bv1, bc1);
    A += (int64_t)blockIdx.z * a_batch;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    const int nk = K / W_BK;
    // the bias loads above are older than every DMA: a counted wait on the DMAs retires them too
#pragma unroll
    for (int s = 0; s < W_STAGES - 1; s++)
        if (s < nk) {
            stage_rows32<G_BM>(A, lda, m0, M - 1, s * W_BK, smem + s * W_STAGE, wv, lane);
            stage_rows32<W_BN>(B, K, n0, N - 1, s * W_BK, smem + s * W_STAGE + G_BM * W_BK, wv, lane);
        }
    int cur = 0;
    for (int kt = 0; kt < nk; kt++) {
        const op_t *sA = smem + cur * W_STAGE, *sB = sA + G_BM * W_BK;
        // K-step kt has landed once at most the DMAs of the one younger stage (3 per wave) are outstanding
        if (W_STAGES > 2 && kt + 1 < nk) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + W_STAGES - 1 < nk) {                            // refill the stage K-step kt-1 has released
            int nx = cur + W_STAGES - 1; if (nx >= W_STAGES) nx -= W_STAGES;
            op_t *nA = smem + nx * W_STAGE;
            stage_rows32<G_BM>(A, lda, m0, M - 1, (kt + W_STAGES - 1) * W_BK, nA, wv, lane);
            stage_rows32<W_BN>(B, K, n0, N - 1, (kt + W_STAGES - 1) * W_BK, nA + G_BM * W_BK, wv, lane);
        }
        opx8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int row = wr * 64 + i * 16 + fr;
            a[i] = *reinterpret_cast<const opx8 *>(&sA[row * W_BK + swz32(row, fq) * 8]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int row = wc * 64 + j * 16 + fr;
            b[j] = *reinterpret_cast<const opx8 *>(&sB[row * W_BK + swz32(row, fq) * 8]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
        cur = cur + 1 == W_STAGES ? 0 : cur + 1;
    }
    float *tile = reinterpret_cast<float *>(smem);               // [128][G_TLD] fp32: one half of the columns per pass
#pragma unroll
    for (int p = 0; p < 2; p++) {
        __syncthreads();                                         // operand reads (p = 0) / the first pass's tile reads are done
        if ((wc >> 1) == p) {
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        tile[(wr * 64 + i * 16 + fq * 4 + r) * G_TLD + (wc & 1) * 64 + j * 16 + fr] = acc[i][j][r];
        }
        __syncthreads();
        if (p == 0) gemm_store_tile<EPI>(tile, tid, m0, n0, M, N, bv0, bc0, Cv, ldc, (int64_t)blockIdx.z * c_batch, pos, pos_T, v_col0, vt_sp);
        else gemm_store_tile<EPI>(tile, tid, m0, n0 + 128, M, N, bv1, bc1, Cv, ldc, (int64_t)blockIdx.z * c_batch, pos, pos_T, v_col0, vt_sp);
    }
}

// ---------------------------------------------------------------------------
// LayerNorm over the last dimension (one wavefront per row)
// ---------------------------------------------------------------------------
// The row is read once with 16-byte loads and kept in registers: NV float4 per lane, so d <= 256 NV.  NV = 5 up to d = 1280 (every width of
// the Whisper / BERT checkpoints: the code and bits that k_xq_fused restates), NV = 8 up to LN_D_MAX; launch_layernorm and launch_add_layernorm
// pick it from d.  Statistics in fp32, two-pass (mean, then centred second moment) as torch does.
template <class OUT> __device__ __forceinline__ void ln_store4(OUT *p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void ln_store4<float>(float *p, float a, float b, float c, float d)
{
    *reinterpret_cast<float4 *>(p) = make_float4(a, b, c, d);
}
template <> __device__ __forceinline__ void ln_store4<op_t>(op_t *p, float a, float b, float c, float d)
{
    typedef __attribute__((ext_vector_type(4))) op_t opx4;
    opx4 v; v[0] = (op_t)a; v[1] = (op_t)b; v[2] = (op_t)c; v[3] = (op_t)d;
    *reinterpret_cast<opx4 *>(p) = v;
}

constexpr int LN_D_MAX = 2048;
template <class OUT, int NV = 5>
__global__ __launch_bounds__(256) void k_layernorm(const float *x, const float *__restrict__ w, const float *__restrict__ b,
                                                  int64_t rows, int d, OUT *__restrict__ out, float eps = 1e-5f, float *out2 = nullptr, int round_in16 = 0,
                                                  op_t *__restrict__ in16_out = nullptr)
{   // out2 (optional, may alias x): the same values in fp32 -- the post-LN residual stream of the BERT layers
    // round_in16: the input is taken as rounded to op_t (the first LayerNorm of the encoder in the 16-bit-stream mode: the reference's stem output
    // IS fp16 -- gelu(conv2) + positional embedding in half precision -- and k_add_layernorm's first-layer form rounds the same values the same way)
    // in16_out (with round_in16): the rounded input itself, as op_t rows -- the 16-bit residual stream the GEMM epilogues of layer 0 add to
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float4 *xr = reinterpret_cast<const float4 *>(x + row * d);
    const int nv = d >> 2;                               // float4 per row, d % 4 == 0
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int idx = lane + 64 * i;
        v[i] = idx < nv ? xr[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (round_in16) v[i] = make_float4((float)(op_t)v[i].x, (float)(op_t)v[i].y, (float)(op_t)v[i].z, (float)(op_t)v[i].w);
        if (in16_out && idx < nv) ln_store4<op_t>(in16_out + row * d + 4 * idx, v[i].x, v[i].y, v[i].z, v[i].w);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    s = wave_dpp_sum_f32(s);
    const float mean = s / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        if (lane + 64 * i < nv) {
            const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    }
    q = wave_dpp_sum_f32(q);
    const float inv = rsqrtf(q / (float)d + eps);
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int idx = lane + 64 * i;
        if (idx < nv) {
            const float4 ww = reinterpret_cast<const float4 *>(w)[idx], bb = reinterpret_cast<const float4 *>(b)[idx];
            const float y0 = (v[i].x - mean) * inv * ww.x + bb.x, y1 = (v[i].y - mean) * inv * ww.y + bb.y,
                        y2 = (v[i].z - mean) * inv * ww.z + bb.z, y3 = (v[i].w - mean) * inv * ww.w + bb.w;
            ln_store4<OUT>(out + row * d + 4 * idx, y0, y1, y2, y3);
            if (out2) ln_store4<float>(out2 + row * d + 4 * idx, y0, y1, y2, y3);
        }
    }
}

#include "pce_gemm256.inc"

// ---------------------------------------------------------------------------
// attention forward, transposed formulation (attn_block16 below).
//   S^T = K Q^T   (keys on the accumulator rows, queries on its columns = lanes)
//   O^T = V^T P^T (P^T is consumed straight out of the S^T accumulator registers as the B operand: no LDS round trip, no
//                  cross-lane softmax reductions except the exchanges between lane groups)
// One workgroup = 4 waves x 32 queries of one (clip, head); K [64 keys][64 d] and V^T [64 d][64 keys]
// tiles stream through LDS by DMA (global_load_lds), double buffered, XOR-swizzled like the GEMM operands.
// ---------------------------------------------------------------------------
constexpr int AT_QB = 128;                  // queries per workgroup

struct AttnArgs {
    const op_t *q; int64_t q_ld;            // query row i of clip c: q + (q_row0[c] + i) * q_ld + head * 64
    const op_t *k; int64_t k_ld;            // key row j:             k + (k_row0[c] + j) * k_ld + head * 64
    const op_t *vt; int64_t vt_clip; int vt_sp;   // V^T: vt + c * vt_clip + (head * 64 + d) * vt_sp + j
    const int *q_row0, *q_len, *k_row0, *k_len;   // per clip
    op_t *out; int64_t out_ld;              // out + (q_row0[c] + i) * out_ld + head * 64
    int causal;                             // key j visible to query i only if j <= i
    int *fell_back;                         // (self-test only, else null) counts the workgroups of k_attention_lean16 that re-ran on the exact path
};

// ---------------------------------------------------------------------------
// The tile loop (round 4, first on v_mfma_f32_32x32x16 as k_attention_lean): less than half of k_attention's vector instructions per tile.  Per 64-key tile a wave issues
// 16 MFMAs and, in k_attention, about 200 VALU instructions; MFMAs and VALU instructions of all waves of a SIMD share one issue port
// (v_fma 4 cycles, v_exp 8, an MFMA 8 of its 32: MI355X_MICROARCH.md "vector-instruction ISSUE cost"), and with three waves per SIMD the
// PMC counters put k_attention's issue port at 96 % busy (SQ_ACTIVE_INST_ANY / SQ_WAVE_CYCLES = 0.32 per wave): it is instruction-count
// bound.  Removed from the tile loop:
//   * the running maximum.  exp2(s c - m) needs SOME reference m per query, not the maximum: softmax is invariant under the choice and
//     fp32 / op_t share an 8-bit exponent, so with m fixed at the query's maximum over TILE 0 nothing is lost until a later score exceeds
//     m by 127 / c.  That is detected (a non-finite row sum) and the workgroup then runs again on the exact path (EXACT = true: running
//     maximum, accumulator rescale, VALU row sums) -- never on Whisper's logits; tests drive it with synthetic ones and force it;
//   * the row sums: a 17th..20th MFMA per tile against a constant "row 0 = ones" fragment accumulates sum_j P[q][j] in the matrix pipe
//     (which has slack) instead of 32 v_add / 16 v_pk_add (which has none); the sums are over the op_t P the second product consumes;
//   * address arithmetic: K / V^T tiles arrive by LDS-DMA through buffer resources (constant per-lane offsets, one scalar offset per
//     tile; rows past the last key read as zeros and are masked like any invisible key), fragment addresses are loop invariants.
// Same workgroup shape, ring and register budget as k_attention (4 waves x 32 queries, 3 slots = 48 KB, three workgroups per CU).
// Measured, 256 clips x 12 heads x 1500^2: 2.56 -> 2.25 ms per launch.  Tried on the way and dropped: the next tile's S^T MFMAs
// interleaved with this tile's exponentials inside one wave (two score sets in registers, 4 slots, two workgroups per CU): 2.59 ms with or
// without the instruction diet -- waves then wait on LDS-DMA / barriers (SQ_WAIT_ANY 0.41) with too few partners to cover them; the same
// with eight waves per workgroup (half the DMA instructions per wave): 3.0 ms.
// ---------------------------------------------------------------------------
// attn_block16 (round 5): the same workgroup (4 waves x 32 queries, 64-key tiles, the same ring, the same staging instructions) on
// v_mfma_f32_16x16x32.  Why: (a) the row-sum products against the "row 0 = ones" fragment waste 15 of 16 rows instead of 31 of 32 -- 4
// MFMAs of 16 cycles per tile instead of 4 of 32, and the ablation of round 4 priced those four at 5.5 of the kernel's 30.8 ms per step;
// (b) MI355X_MICROARCH.md "DVFS give-back (7)": under the power limit these kernels run against, the 16x16x32 loop holds a higher clock.
// Per tile and wave: 16 MFMAs for S^T (4 key blocks x 2 query blocks x 2 k-steps of 32 dims), 16 for O^T += V^T P^T (4 d blocks x 2
// query blocks x 2 k-steps of 32 keys), 4 for the row sums: 576 MFMA cycles against 640.
// Layouts.  D = A B of 16x16x32: lane (n = lane & 15, g = lane >> 4) supplies A[m = n][8g .. 8g + 7] and B[8g .. 8g + 7][n], and holds
// D[4g + i][n] in register i.  S^T block (kb, qb) therefore leaves, in lane (query n, group g), the scores of the four keys on block rows
// 4g .. 4g + 3; the B operand of the second product wants, in the same lane, eight keys of one 32-key k-step.  Registers of blocks kb = 2s
// and 2s + 1 concatenated ARE such an operand if block row rho = 4g + i of block 2s + b stands for key 32s + 8g + 4b + i: the K rows are
// staged into LDS in that order (the LDS-DMA source row is free per lane: row R of the slot holds key kappa(R)), so the K fragments are
// read from natural, conflict-free rows and the V^T fragment of lane (d, g) is one contiguous 16-byte read of keys 32s + 8g .. + 7.
// No cross-lane movement, no LDS round trip for P.  Softmax does not care about the order of the keys inside a tile.
// ---------------------------------------------------------------------------
template <bool EXACT, bool NT>
__device__ __forceinline__ bool attn_block16(const AttnArgs &A, op_t *smem, int bx, int head, int clip)
{
    constexpr int NS = 3, DPW = 4;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, g = lane >> 4;
    const int Sq = A.q_len[clip], Sk = A.k_len[clip];
    const int q0 = bx * AT_QB + wv * 32;
    const op_t *qbase = A.q + (int64_t)A.q_row0[clip] * A.q_ld + head * 64;
    const op_t *kbase = A.k + (int64_t)A.k_row0[clip] * A.k_ld + head * 64;
    const op_t *vtbase = A.vt + (int64_t)clip * A.vt_clip + (int64_t)head * 64 * A.vt_sp;
    const int kld = (int)A.k_ld, vsp = A.vt_sp;
    const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(const_cast<op_t *>(kbase), 0, ((Sk - 1) * kld + 64) * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(const_cast<op_t *>(vtbase), 0, 64 * vsp * 2, 0x00020000);
    int voffK[2], voffV[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int row = (wv + 4 * i) * 8 + (lane >> 3), c8 = swz_chunk(row, lane & 7) * 8;
        const int kb = row >> 4, rho = row & 15;
        const int key = 32 * (kb >> 1) + 8 * (rho >> 2) + 4 * (kb & 1) + (rho & 3);     // kappa(row): the key LDS row `row` of a K slot holds
        voffK[i] = (key * kld + c8) * 2; voffV[i] = (row * vsp + c8) * 2;
    }
    auto stage = [&](int t) {
        op_t *sK = smem + (t % NS) * (2 * 64 * 64), *sV = sK + 64 * 64;
        const int key0 = t * 64;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            // NT: a launch with ONE query block per (clip, head) -- the decoder's cross-attention -- reads every K / V^T byte exactly once: the
            // non-temporal policy (sc0 | nt) streams them past the caches (profiles/r05/xattn_absorb.txt: +14 % on such a stream)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, (__attribute__((address_space(3))) void *)(sK + (wv + 4 * i) * 8 * 64), 16, voffK[i], key0 * kld * 2, 0, NT ? 3 : 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (__attribute__((address_space(3))) void *)(sV + (wv + 4 * i) * 8 * 64), 16, voffV[i], key0 * 2, 0, NT ? 3 : 0);
        }
    };
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    opx8 qf[2][2];                                              // [query block][k-step of 32 dims]
    int my_q[2];
#pragma unroll
    for (int qb = 0; qb < 2; qb++) {
        my_q[qb] = q0 + 16 * qb + n16;
        int qr = my_q[qb]; if (qr >= Sq) qr = Sq - 1;
        const op_t *qp = qbase + (int64_t)qr * A.q_ld;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) qf[qb][ks] = *reinterpret_cast<const opx8 *>(qp + 32 * ks + 8 * g);
    }
    opx8 ones;                                                 // A fragment "row 0 = ones, rows 1..15 = 0" of the row-sum MFMA
#pragma unroll
    for (int j = 0; j < 8; j++) ones[j] = (op_t)(n16 == 0 ? 1.0f : 0.0f);
    f32x4 o[4][2], osum[2];
#pragma unroll
    for (int db = 0; db < 4; db++) { o[db][0] = z4; o[db][1] = z4; }
    osum[0] = z4; osum[1] = z4;
    float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
    const float sl2 = 0.125f * 1.4426950408889634f;
    int k_need = Sk;
    if (A.causal) k_need = min(Sk, bx * AT_QB + AT_QB);
    const int nt = (k_need + 63) / 64;
    int kaddr[4][2], vaddr[4][2];                                // LDS addresses of this lane's fragments inside a slot (elements)
#pragma unroll
    for (int b4 = 0; b4 < 4; b4++)
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const int row = 16 * b4 + n16;
            kaddr[b4][ks] = row * 64 + swz_chunk(row, 4 * ks + g) * 8;
            vaddr[b4][ks] = 64 * 64 + row * 64 + swz_chunk(row, 4 * ks + g) * 8;
        }
    stage(0);
    if (nt > 1) stage(1);
    for (int kt = 0; kt < nt; kt++) {
        if (kt + 1 < nt) __builtin_amdgcn_s_waitcnt(0x0F70 | DPW); else __builtin_amdgcn_s_waitcnt(0x0F70 | 0);
        __builtin_amdgcn_s_barrier();
        if (kt + 2 < nt) stage(kt + 2);
        const op_t *sC = smem + (kt % NS) * (2 * 64 * 64);
        f32x4 sc[4][2];
#pragma unroll
        for (int kb = 0; kb < 4; kb++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                const opx8 kf = *reinterpret_cast<const opx8 *>(&sC[kaddr[kb][ks]]);
#pragma unroll
                for (int qb = 0; qb < 2; qb++) sc[kb][qb] = mfma16(kf, qf[qb][ks], ks == 0 ? z4 : sc[kb][qb]);
            }
        if ((kt * 64 + 63 >= Sk) || (A.causal && kt * 64 + 63 > q0)) {                          // wave-uniform: an edge tile
#pragma unroll
            for (int kb = 0; kb < 4; kb++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int key = kt * 64 + 32 * (kb >> 1) + 8 * g + 4 * (kb & 1) + i;
#pragma unroll
                    for (int qb = 0; qb < 2; qb++) {
                        const bool vis = key < Sk && (!A.causal || key <= my_q[qb]);
                        sc[kb][qb][i] = vis ? sc[kb][qb][i] : -1e30f;
                    }
                }
        }
        if (EXACT || kt == 0) {
            float mx[2];
#pragma unroll
            for (int qb = 0; qb < 2; qb++) {
                float m = sc[0][qb][0];
#pragma unroll
                for (int kb = 0; kb < 4; kb++)
#pragma unroll
                    for (int i = 0; i < 4; i++) m = fmaxf(m, sc[kb][qb][i]);
                m = m > -1e29f ? m * sl2 : -1e30f;
                m = fmaxf(m, __shfl_xor(m, 16, 64));
                m = fmaxf(m, __shfl_xor(m, 32, 64));
                mx[qb] = fmaxf(m_run[qb], m);
            }
            if (__builtin_amdgcn_ballot_w64(mx[0] > m_run[0] || mx[1] > m_run[1]) != 0) {
#pragma unroll
                for (int qb = 0; qb < 2; qb++) {
                    const float corr = __builtin_amdgcn_exp2f(m_run[qb] - mx[qb]);   // (tile 0: everything it scales is still zero)
                    l_run[qb] *= corr;
#pragma unroll
                    for (int db = 0; db < 4; db++)
#pragma unroll
                        for (int i = 0; i < 4; i++) o[db][qb][i] *= corr;
                    m_run[qb] = mx[qb];
                }
            }
            // fp16 operands: P = 2^(s c - m) must stay below 65 504 = 2^16 (bf16 has fp32's exponent range).  The fixed reference sits
            // 4 octaves ABOVE the first tile's maximum: a later score may exceed that maximum by 2^20 (13.9 nats) before the row overflows
            // (and the workgroup re-runs exactly), at the price of flushing weights below 2^-20 of the reference to zero
            // (<= 1 500 keys x 1e-6: 0.15 % of a row in the worst case; the exact path, like the reference, cuts at 2^-24).
            if (!EXACT && std::is_same<op_t, _Float16>::value) { m_run[0] += 4.0f; m_run[1] += 4.0f; }
        }
        float rs[2] = {0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; kb++)
#pragma unroll
            for (int qb = 0; qb < 2; qb++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(sc[kb][qb][i], sl2, -m_run[qb]));
                    sc[kb][qb][i] = pv;
                    if (EXACT) rs[qb] += pv;
                }
        if (EXACT) {
#pragma unroll
            for (int qb = 0; qb < 2; qb++) {
                float sum = rs[qb];
                sum += __shfl_xor(sum, 16, 64);
                sum += __shfl_xor(sum, 32, 64);
                l_run[qb] += sum;
            }
        }
        // O^T += V^T P^T (and the row sums): k-step s covers keys 32 s .. 32 s + 31; B = the registers of S^T blocks 2 s and 2 s + 1
        opx8 vf[4][2];
#pragma unroll
        for (int db = 0; db < 4; db++)
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) vf[db][s2] = *reinterpret_cast<const opx8 *>(&sC[vaddr[db][s2]]);
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
            for (int qb = 0; qb < 2; qb++) {
                opx8 pf;
#pragma unroll
                for (int i = 0; i < 4; i++) { pf[i] = (op_t)sc[2 * s2][qb][i]; pf[4 + i] = (op_t)sc[2 * s2 + 1][qb][i]; }
#pragma unroll
                for (int db = 0; db < 4; db++) o[db][qb] = mfma16(vf[db][s2], pf, o[db][qb]);
                if (!EXACT) osum[qb] = mfma16(ones, pf, osum[qb]);
            }
    }
    if (!EXACT) {                                               // row 0 of the row-sum product: register 0 of lanes 0..15
        l_run[0] = __shfl(osum[0][0], n16, 64);
        l_run[1] = __shfl(osum[1][0], n16, 64);
    }
    const bool ok = EXACT || (((l_run[0] > 0.f && l_run[0] < 1.0e30f) || my_q[0] >= Sq) && ((l_run[1] > 0.f && l_run[1] < 1.0e30f) || my_q[1] >= Sq));
    if (!EXACT && __syncthreads_or(!ok)) return false;           // some row overflowed its fixed reference: the workgroup runs again, exactly
    // O^T block (db, qb): this lane holds d = 16 db + 4 g .. + 3 of query q0 + 16 qb + n16
    typedef __attribute__((ext_vector_type(4))) op_t opx4;
#pragma unroll
    for (int qb = 0; qb < 2; qb++) {
        if (my_q[qb] >= Sq) continue;
        const float inv = 1.0f / l_run[qb];
        op_t *op = A.out + ((int64_t)A.q_row0[clip] + my_q[qb]) * A.out_ld + head * 64;
#pragma unroll
        for (int db = 0; db < 4; db++) {
            opx4 v4;
#pragma unroll
            for (int i = 0; i < 4; i++) v4[i] = (op_t)(o[db][qb][i] * inv);
            *reinterpret_cast<opx4 *>(op + 16 * db + 4 * g) = v4;
        }
    }
    return true;
}

// Workgroups go to the 8 XCDs round robin by linear id, and the query blocks of one (clip, head) share its K / V^T through L2: every XCD gets a
// CONTIGUOUS range of (clip, head, query block) triples, so that the blocks that share keys meet in one L2 instead of eight.
// NT: a launch with one query block per (clip, head) (see attn_block16's staging).
template <bool NT>
__global__ __launch_bounds__(256, 3) void k_attention_lean16(AttnArgs A, int force_exact /* self-test only */)
{
    __shared__ __attribute__((aligned(1024))) op_t smem[3 * 2 * 64 * 64];
    const unsigned nx = gridDim.x, ny = gridDim.y, total = nx * ny * gridDim.z;
    const unsigned lin = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z), xcd = lin & 7u, per = total >> 3, rem = total & 7u;
    const unsigned logical = xcd * per + (xcd < rem ? xcd : rem) + (lin >> 3);
    const int bx = (int)(logical % nx), head = (int)((logical / nx) % ny), clip = (int)(logical / (nx * ny));
    if (bx * AT_QB >= A.q_len[clip]) return;
    if (!force_exact && attn_block16<false, NT>(A, smem, bx, head, clip)) return;
    if (!force_exact && A.fell_back && threadIdx.x == 0) atomicAdd(A.fell_back, 1);
    __syncthreads();
    attn_block16<true, NT>(A, smem, bx, head, clip);
}

static void launch_attention(pce_ctx *c, dim3 grid, const AttnArgs &a, double flops = 0.0, int force_exact = 0 /* self-test only */)
{
    // flops > 0: a launch the profiler brackets on its own (the encoder's); the decoder's small launches stay inside their composite entry
    KernelTimer kt(c, PCE_K_ATTENTION_LEAN, nullptr, flops);
    if (grid.x == 1) hipLaunchKernelGGL(k_attention_lean16<true>, grid, dim3(256), 0, c->stream, a, force_exact);
    else hipLaunchKernelGGL(k_attention_lean16<false>, grid, dim3(256), 0, c->stream, a, force_exact);
}
// The product's attention launch (the one place it fills an AttnArgs): H heads of n clips, up to q_rows queries each, out rows of H * 64
static void launch_attention_rows(pce_ctx *c, int n, int H, int q_rows, const op_t *q, int64_t q_ld, const op_t *k, int64_t k_ld, const op_t *vt, int vt_sp,
                                  const int *q_row0, const int *q_len, const int *k_row0, const int *k_len, op_t *out, int causal, double flops = 0.0)
{
    AttnArgs a{};
    a.q = q; a.q_ld = q_ld; a.k = k; a.k_ld = k_ld; a.vt = vt; a.vt_clip = (int64_t)H * 64 * vt_sp; a.vt_sp = vt_sp;
    a.q_row0 = q_row0; a.q_len = q_len; a.k_row0 = k_row0; a.k_len = k_len; a.out = out; a.out_ld = H * 64; a.causal = causal;
    launch_attention(c, dim3((unsigned)div_up(q_rows, AT_QB), (unsigned)H, (unsigned)n), a, flops);
}

// ---------------------------------------------------------------------------
// Text decoder (teacher forced) and cross-attention alignment  -- openai-whisper timing.py find_alignment
// ---------------------------------------------------------------------------
__global__ void k_embed_tokens(const int *__restrict__ tokens /* [clips][T_pad] */, const float *__restrict__ tok_emb,
                               const float *__restrict__ pos_emb, int T_pad, int n_ctx, int d, int64_t rows, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * d) return;
    const int64_t m = i / d; const int col = (int)(i - m * d);
    int t = (int)(m % T_pad); if (t >= n_ctx) t = n_ctx - 1;      // pad rows beyond the clip's tokens: any finite value
    out[i] = tok_emb[(int64_t)tokens[m] * d + col] + pos_emb[(int64_t)t * d + col];
}

// last position of every sequence: resid row (clip * T_pad + len - 1) -> out row clip
__global__ void k_gather_last(const float *__restrict__ resid, const int *__restrict__ t_len, int T_pad, int d, int n, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * d) return;
    const int clip = (int)(i / d), col = (int)(i - (int64_t)clip * d);
    out[i] = resid[((int64_t)clip * T_pad + t_len[clip] - 1) * d + col];
}

// self-attention cache maintenance.  k_cache_k: K rows of a prefix run, [clip * T_pad + t][2d] (second half) -> cache
// [clip][T_cap][d] (an incremental step's attention kernel appends its new position itself).
__global__ void k_cache_k(const op_t *__restrict__ qk, int T_pad, const int *__restrict__ t_len, int d, int T_cap, int n, op_t *__restrict__ ck)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * T_pad * d) return;
    const int col = (int)(i % d); const int64_t r = i / d; const int t = (int)(r % T_pad), clip = (int)(r / T_pad);
    if (t < t_len[clip]) ck[((int64_t)clip * T_cap + t) * d + col] = qk[r * 2 * d + d + col];
}
// V rows of a prefix run for the incremental steps' self-attention: V^T image [clip][d][sp] (written by the QKV epilogue) -> row-major [clip][T_cap][d]
__global__ void k_cache_v_rows(const op_t *__restrict__ cvt, const int *__restrict__ t_len, int d, int T_cap, int sp, int n, op_t *__restrict__ cv)
{
    __shared__ op_t t[32][33];
    const int clip = blockIdx.z, c0 = blockIdx.x * 32, t0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int T = t_len[clip];
    if (t0 >= T) return;
    for (int r = ty; r < 32; r += 8) t[r][tx] = cvt[((int64_t)clip * d + c0 + r) * sp + t0 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (t0 + r < T) cv[((int64_t)clip * T_cap + t0 + r) * d + c0 + tx] = t[tx][r];
}

// Self-attention of an incremental decoding step on ROW-MAJOR caches (K rows and V rows [clip][T_cap][d]): one wave per (clip, head), one
// workgroup per clip.  Appending the new position is two coalesced 128-byte row stores per wave -- the V^T image of the prefix kernels would take
// 64 two-byte stores at a 1 KB stride, which was a third of this launch (profiles/r05/xattn_absorb.txt).  Scores as k_cross_attn1w computes them
// (8 lanes per key row, eight rows per lane in flight, fp32 softmax in LDS); the weighted sum over V walks the rows the same way, every lane
// accumulating its 8 dimensions over the keys of its group, the eight groups added by shuffles.  The new key / value are attended to from registers.
struct SelfAttn1Args {
    const op_t *qkv; int64_t qkv_ld;          // the new position: q | k | v of clip c at qkv + c * qkv_ld (+ d, + 2 d)
    op_t *ck, *cv; int64_t c_clip; int d;     // caches: row t of clip c at + c * c_clip + t * d
    const int *pos, *skip;                    // position of the new token (= cached keys) per clip; skip may be null
    op_t *out; int64_t out_ld;
    int heads;
};
// More than 16 heads (large-v3 / turbo: 20): the heads are cut into groups of at most 16 waves, one workgroup per (clip, group) -- grid (clips, groups),
// wave w of group y is head y * (waves per group) + w; each wave appends its own head's columns.  Up to 16 heads: one group, the launch of round 5.
__global__ __launch_bounds__(1024) void k_self_attn1w(SelfAttn1Args A)
{
    extern __shared__ float sa_sp[];                              // [waves of the group][512]
    const int clip = blockIdx.x;
    if (A.skip && A.skip[clip]) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = (int)blockIdx.y * (int)(blockDim.x >> 6) + wv;
    if (head >= A.heads) return;                                  // (a short last group; no barrier in this kernel)
    float *sp = sa_sp + wv * 512;
    const int Sc = A.pos[clip];                                   // cached keys 0 .. Sc - 1; the new one is key Sc
    const int g = lane >> 3, ch = lane & 7;
    const op_t *nq = A.qkv + (int64_t)clip * A.qkv_ld + head * 64;
    const opx8 qv = *reinterpret_cast<const opx8 *>(nq + ch * 8);
    const opx8 k_new = *reinterpret_cast<const opx8 *>(nq + A.d + ch * 8), v_new = *reinterpret_cast<const opx8 *>(nq + 2 * A.d + ch * 8);
    const op_t kn = nq[A.d + lane], vn = nq[2 * A.d + lane];
    op_t *ckb = A.ck + (int64_t)clip * A.c_clip + head * 64, *cvb = A.cv + (int64_t)clip * A.c_clip + head * 64;
    ckb[(int64_t)Sc * A.d + lane] = kn;                           // (nothing in this launch reads row Sc back)
    cvb[(int64_t)Sc * A.d + lane] = vn;
    float qf[8];
#pragma unroll
    for (int e = 0; e < 8; e++) qf[e] = (float)qv[e] * 0.125f;
    constexpr int U = 8;
    float m = -3.0e38f;
    for (int base = 0; base < Sc; base += 8 * U) {
        opx8 kv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = base + u * 8 + g;
            kv[u] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(ckb + (int64_t)(r < Sc ? r : Sc - 1) * A.d + ch * 8));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            float dd = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) dd = fmaf((float)kv[u][e], qf[e], dd);
            dd += __shfl_xor(dd, 1, 64); dd += __shfl_xor(dd, 2, 64); dd += __shfl_xor(dd, 4, 64);
            const int r = base + u * 8 + g;
            if (r < Sc) { m = fmaxf(m, dd); if (ch == 0) sp[r] = dd; }
        }
    }
    float s_new;
    {
        float dd = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) dd = fmaf((float)k_new[e], qf[e], dd);
        dd += __shfl_xor(dd, 1, 64); dd += __shfl_xor(dd, 2, 64); dd += __shfl_xor(dd, 4, 64);
        s_new = dd; m = fmaxf(m, dd);
    }
    m = wave_xor_max(m);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    float sum = 0.f;
    for (int t = lane; t < Sc; t += 64) {
        const float pv = __expf(sp[t] - m);
        sp[t] = pv; sum += pv;
    }
    sum = wave_xor_sum(sum);
    const float p_new = __expf(s_new - m);                       // (the same value in every lane)
    sum += p_new;
    const float inv = 1.0f / sum;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] = 0.f;
    for (int base = 0; base < Sc; base += 8 * U) {
        opx8 vv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = base + u * 8 + g;
            vv[u] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(cvb + (int64_t)(r < Sc ? r : Sc - 1) * A.d + ch * 8));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = base + u * 8 + g;
            const float wgt = r < Sc ? sp[r] : 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] = fmaf(wgt, (float)vv[u][e], acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
        float a = acc[e];
        a += __shfl_xor(a, 8, 64); a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
        acc[e] = fmaf(p_new, (float)v_new[e], a) * inv;
    }
    if (g == 0) {
        opx8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (op_t)acc[e];
        *reinterpret_cast<opx8 *>(A.out + (int64_t)clip * A.out_ld + head * 64 + ch * 8) = o;
    }
}
__global__ void k_embed_one(const int *__restrict__ tok, const float *__restrict__ tok_emb, const float *__restrict__ pos_emb,
                            const int *__restrict__ pos_of, int d, int n, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * d) return;
    const int clip = (int)(i / d), col = (int)(i - (int64_t)clip * d);
    out[i] = tok_emb[(int64_t)tok[clip] * d + col] + pos_emb[(int64_t)pos_of[clip] * d + col];
}

// ---- device-resident decoding loop (round 3) -----------------------------------------------------------------------------------
// After the logit filters have chosen `next` for every sequence, k_step_advance appends it to the device-resident token table,
// refreshes the per-sequence tables the NEXT step's kernels read (new token, position, self-attention key count, "ended" flag),
// records the step's outputs and counts the sequences whose last token is end-of-text.  Nothing of a step passes through the host.
// tables ct[8 n]: new token | q_row0 | q_len | k_row0 | k_len | a_row0 | a_len | position   (the layout pce_whisper_decode_step_ex uploads)
__global__ __launch_bounds__(256) void k_step_advance(int n, int T_cap, int eot, int max_new, int *__restrict__ tok_table, int *__restrict__ len,
                                                     const int *__restrict__ next, const float *__restrict__ next_lp, int *__restrict__ ct,
                                                     int *__restrict__ ended, int *__restrict__ out_tok, float *__restrict__ out_lp,
                                                     int *__restrict__ step_ctr, int *__restrict__ n_ended)
{   // ONE workgroup (a few hundred sequences)
    const int step = *step_ctr;
    __syncthreads();
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int L = len[i], t = next[i];
        if (step < max_new) { out_tok[(size_t)i * max_new + step] = t; out_lp[(size_t)i * max_new + step] = next_lp[i]; }
        // L == T_cap: `t` followed a forward pass over the FULL text context; it is reported (out_tok above) but cannot be fed back.  The
        // sequence stops here, the reference's `tokens.shape[-1] > n_ctx: break`: the last table entry becomes end-of-text so that every later
        // step reads the sequence as ended (its real value has already left through out_tok one step earlier).
        if (L < T_cap) { tok_table[(size_t)i * T_cap + L] = t; len[i] = L + 1; }
        else tok_table[(size_t)i * T_cap + T_cap - 1] = eot;
        ct[i] = t; ct[4 * n + i] = (L < T_cap ? L : T_cap - 1) + 1; ct[7 * n + i] = L < T_cap ? L : T_cap - 1;
        const int e = t == eot || L >= T_cap;
        ended[i] = e; cnt += e;
    }
    if (cnt) atomicAdd(n_ended + (step < max_new ? step : max_new - 1), cnt);
    if (threadIdx.x == 0) *step_ctr = step + 1;
}

// Attention of ONE query per (clip, head) over a long key axis: the cross-attention (1 500 audio positions) and the cached
// self-attention of an incremental decoding step.  The MFMA attention kernels spend a 32-query tile on it and walk the keys as 24
// dependent LDS-DMA tiles per workgroup; this is a streaming kernel: HBM-bound by construction (one pass over K, one over V^T:
// 14 GB per step for 256 clips at Whisper-small size, the roofline of free-running decoding).
//   phase 1: scores.  8 lanes per key row (16 B = 8 dims each: a wave-instruction covers eight whole 128-byte lines), eight rows per lane
//            in flight, 8-lane sums by DPP -> fp32 scores in LDS
//   phase 2: softmax (fp32, max-subtracted) in LDS
//   phase 3: O[d] = sum_t p[t] V^T[d][t]: the wave streams the V^T rows of its head as 1 KB pieces (lane = 8 consecutive keys, p in registers)
// `skip[clip]` != 0: the sequence has ended, its output is never used (the filters return end-of-text for it): no bytes are read.
struct Attn1Args {
    const op_t *q; int64_t q_ld;              // query of clip c: q + c * q_ld + head * 64
    const op_t *k; int64_t k_ld;              // key row j:       k + (k_row0[c] + j) * k_ld + head * 64
    const op_t *vt; int64_t vt_clip; int vt_sp;   // V^T:        vt + c * vt_clip + (head * 64 + d) * vt_sp + j   (columns >= k_len hold finite values)
    const int *k_row0, *k_len;                // per clip; k_len <= 1536
    const int *skip;                          // per clip or null
    op_t *out; int64_t out_ld;                // out + c * out_ld + head * 64
    // when app_pos is set, the wave of (clip, head) first writes the new position's key / value slice (app_k / app_v + c * app_ld + head * 64)
    // into K row app_pos[c] and V^T column app_pos[c], then attends
    const op_t *app_k, *app_v; int64_t app_ld; const int *app_pos;
    int heads;                                // heads in all (the grid's y counts head groups)
};
// k_cross_attn1w: ONE WAVE per (clip, head) and one workgroup per clip (wave = head).  Why: a key row is the
// 128-byte slices of all heads side by side (1 536 B at Whisper-small size); with a workgroup per (clip, head) the twelve slices of a row
// are fetched by twelve workgroups on different XCDs at different times -- twelve visits to the same DRAM page; here the waves of a
// workgroup walk the rows together.  Each wave keeps its scores in its own LDS slice: no workgroup barrier anywhere.
// More than 16 heads: groups of at most 16 waves, grid (clips, groups), as k_self_attn1w.
__global__ __launch_bounds__(1024) void k_cross_attn1w(Attn1Args A)
{
    extern __shared__ float spw[];                               // [waves of the group][1536 + 64]
    const int clip = blockIdx.x;
    if (A.skip && A.skip[clip]) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = (int)blockIdx.y * (int)(blockDim.x >> 6) + wv;
    if (head >= A.heads) return;                                  // (a short last group)
    float *sp = spw + wv * 1600;
    const int Sk = A.k_len[clip];
    const int g = lane >> 3, ch = lane & 7;
    // Appending (the self-attention of an incremental step): the new position's key and value go to the cache with plain stores that
    // nothing in this launch reads back -- the wave attends to the new key from registers (its score from the key slice it has just
    // loaded, its value added after the sums over the cached keys), so there is no store -> wait -> load chain (that chain cost as much
    // as the separate append launch it replaced: 7 us).  The V^T cache only ever holds finite values (zeroed at allocation).
    const bool app = A.app_pos != nullptr;
    const int pos = app ? A.app_pos[clip] : 0;                    // == Sk - 1 when appending
    const int Sc = app ? Sk - 1 : Sk;                             // keys read from memory
    float v_new = 0.f;
    opx8 k_new;
#pragma unroll
    for (int e = 0; e < 8; e++) k_new[e] = (op_t)0.f;
    if (app) {
        const op_t kn = A.app_k[(int64_t)clip * A.app_ld + head * 64 + lane], vn = A.app_v[(int64_t)clip * A.app_ld + head * 64 + lane];
        const_cast<op_t *>(A.k)[((int64_t)A.k_row0[clip] + pos) * A.k_ld + head * 64 + lane] = kn;
        const_cast<op_t *>(A.vt)[(int64_t)clip * A.vt_clip + (int64_t)(head * 64 + lane) * A.vt_sp + pos] = vn;
        v_new = (float)vn;
        k_new = *reinterpret_cast<const opx8 *>(A.app_k + (int64_t)clip * A.app_ld + head * 64 + ch * 8);
    }
    float qf[8];
    {
        const opx8 qv = *reinterpret_cast<const opx8 *>(A.q + (int64_t)clip * A.q_ld + head * 64 + ch * 8);
#pragma unroll
        for (int e = 0; e < 8; e++) qf[e] = (float)qv[e] * 0.125f;
    }
    const op_t *kb = A.k + (int64_t)A.k_row0[clip] * A.k_ld + head * 64 + ch * 8;
    constexpr int U = 8;
    float m = -3.0e38f;
    for (int base = 0; base < Sc; base += 8 * U) {
        opx8 kv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = base + u * 8 + g;
            kv[u] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(kb + (int64_t)(r < Sc ? r : Sc - 1) * A.k_ld));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) d = fmaf((float)kv[u][e], qf[e], d);
            d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
            const int r = base + u * 8 + g;
            if (r < Sc) { m = fmaxf(m, d); if (ch == 0) sp[r] = d; }
        }
    }
    if (app) {                                                    // the new key, scored the same way (same operation order as a cached row)
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) d = fmaf((float)k_new[e], qf[e], d);
        d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
        m = fmaxf(m, d);
        if (lane == 0) sp[pos] = d;
    }
    m = wave_xor_max(m);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    float sum = 0.f;
    const int Sp = (Sk + 511) & ~511;
    for (int t = lane; t < Sp; t += 64) {
        const float pv = t < Sk ? __expf(sp[t] - m) : 0.f;
        sp[t] = pv; sum += pv;
    }
    sum = wave_xor_sum(sum);
    const float inv = 1.0f / sum;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    const int np = Sp >> 9;
    const float p_new = app ? sp[pos] : 0.f;                     // weight of the new key
    if (Sk <= 128) {
        // few keys (the self-attention of a decoding step): lane d owns output dimension d and reads the first Sk keys of ITS V^T row, all
        // sixteen 16-byte loads requested at once -- one memory round trip.  (The general form below walks the 64 rows four at a time:
        // sixteen dependent round trips, 42-51 us per launch for a few dozen keys.)
        const op_t *vr = A.vt + (int64_t)clip * A.vt_clip + (int64_t)(head * 64 + lane) * A.vt_sp;
        opx8 vv[16];
#pragma unroll
        for (int cc = 0; cc < 16; cc++) {
#pragma unroll
            for (int e = 0; e < 8; e++) vv[cc][e] = (op_t)0.f;
            if (cc * 8 < Sk) vv[cc] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(vr + cc * 8));
        }
        float a = 0.f;
#pragma unroll
        for (int cc = 0; cc < 16; cc++)
            if (cc * 8 < Sk) {                                   // (wave-uniform)
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int t = cc * 8 + e;
                    const float wgt = (app && t == pos) ? 0.f : sp[t];      // (column `pos` is being written by this very launch: weight 0; sp[t] = 0 beyond the last key)
                    a = fmaf(wgt, (float)vv[cc][e], a);
                }
            }
        if (app) a = fmaf(p_new, v_new, a);
        A.out[(int64_t)clip * A.out_ld + head * 64 + lane] = (op_t)(a * inv);
        return;
    }
    float pr[3][8];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int t = j * 512 + lane * 8 + e;
            pr[j][e] = (j < np && !(app && t == pos)) ? sp[t] : 0.f;     // (the cached column `pos` is being written by this very launch: weight 0)
        }
    const op_t *vb = A.vt + (int64_t)clip * A.vt_clip + (int64_t)(head * 64) * A.vt_sp + lane * 8;
    const int v_new_bits = __builtin_bit_cast(int, v_new);
    float keep = 0.f;                                            // lane d ends up with output dimension d
#pragma unroll 2
    for (int r4 = 0; r4 < 64; r4 += 4) {
        // a lane whose eight keys all lie beyond the last key does not load (its weights are zero): the self-attention of a decoding step
        // has a few dozen keys in a 512-column image -- reading whole rows cost 200 MB and ~50 us per launch for 20 MB of live values
        opx8 vv[4][3];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
#pragma unroll
                for (int e = 0; e < 8; e++) vv[r][j][e] = (op_t)0.f;
                if (j < np && j * 512 + lane * 8 < Sk) vv[r][j] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(vb + (int64_t)(r4 + r) * A.vt_sp + j * 512));
            }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (j < np)
#pragma unroll
                    for (int e = 0; e < 8; e++) a = fmaf(pr[j][e], (float)vv[r][j][e], a);
            a = wave_xor_sum(a);
            if (app) a = fmaf(p_new, __builtin_bit_cast(float, __builtin_amdgcn_readlane(v_new_bits, r4 + r)), a);
            if (lane == r4 + r) keep = a * inv;
        }
    }
    A.out[(int64_t)clip * A.out_ld + head * 64 + lane] = (op_t)keep;
}

// The launches of the two single-query kernels, n clips x H heads (the decoding step and pce_selftest_attn1 make them here).  Up to 16 heads: one
// workgroup per clip, one wave per head (115.8 against 119.6 us per launch with a workgroup per clip and head).  More heads (20 at large-v3 /
// turbo): workgroups of at most 16 waves, grid (clip, head group) -- lds_optins (16 waves' slices) covers the largest group.
static void launch_cross_attn1(pce_ctx *c, int n, int H, const Attn1Args &args)
{
    const int hgroups = (H + 15) / 16, hg_waves = (H + hgroups - 1) / hgroups;
    Attn1Args a = args;
    a.heads = H;
    KernelTimer kt(c, PCE_K_CROSS_ATTN1);
    hipLaunchKernelGGL(k_cross_attn1w, dim3((unsigned)n, (unsigned)hgroups), dim3(64 * (unsigned)hg_waves), (size_t)hg_waves * 1600 * 4, c->stream, a);
}
static void launch_self_attn1(pce_ctx *c, int n, int H, const SelfAttn1Args &args)
{
    const int hgroups = (H + 15) / 16, hg_waves = (H + hgroups - 1) / hgroups;
    SelfAttn1Args a = args;
    a.heads = H;
    KernelTimer kt(c, PCE_K_CROSS_ATTN1);
    hipLaunchKernelGGL(k_self_attn1w, dim3((unsigned)n, (unsigned)hgroups), dim3(64 * (unsigned)hg_waves), (size_t)hg_waves * 512 * 4, c->stream, a);
}

#include "pce_xattn.inc"

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
    if (medfilt_width == 7 && !c->generic_median)
        hipLaunchKernelGGL((k_align_cost<7>), dim3((unsigned)div_up(m.F_pad, 256), (unsigned)N_max, (unsigned)m.n), dim3(256), 0, c->stream,
                           m.w, m.t_len, m.f_len, m.n_sel, m.T_pad, m.F_pad, sot_len, medfilt_width, N_max, cost);
    else
        hipLaunchKernelGGL((k_align_cost<0>), dim3((unsigned)div_up(m.F_pad, 256), (unsigned)N_max, (unsigned)m.n), dim3(256), 0, c->stream,
                           m.w, m.t_len, m.f_len, m.n_sel, m.T_pad, m.F_pad, sot_len, medfilt_width, N_max, cost);
}

__global__ void k_f32_to_bf16(const float *__restrict__ in, op_t *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (op_t)in[i];
}

// librosa.filters.mel(sr=16000, n_fft=400, n_mels) (Slaney scale and normalisation), float32
void mel_filterbank(int n_mels, std::vector<float> &dense)
{
    const double sr = 16000.0, f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    auto hz_to_mel = [&](double f) { return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp; };
    auto mel_to_hz = [&](double m) { return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m; };
    std::vector<double> mel_f((size_t)n_mels + 2), fft_f(W_BINS);
    const double m_lo = hz_to_mel(0.0), m_hi = hz_to_mel(sr / 2);
    for (int i = 0; i < n_mels + 2; i++) mel_f[(size_t)i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
    for (int k = 0; k < W_BINS; k++) fft_f[(size_t)k] = (sr / 2) * k / (W_BINS - 1);
    dense.assign((size_t)n_mels * W_BINS, 0.f);
    for (int i = 0; i < n_mels; i++) {
        const double enorm = 2.0 / (mel_f[(size_t)i + 2] - mel_f[(size_t)i]);
        for (int k = 0; k < W_BINS; k++) {
            const double lower = -(mel_f[(size_t)i] - fft_f[(size_t)k]) / (mel_f[(size_t)i + 1] - mel_f[(size_t)i]);
            const double upper = (mel_f[(size_t)i + 2] - fft_f[(size_t)k]) / (mel_f[(size_t)i + 2] - mel_f[(size_t)i + 1]);
            const double w = std::max(0.0, std::min(lower, upper));
            dense[(size_t)i * W_BINS + k] = (float)(w * enorm);
        }
    }
}

struct WhisperState {
    pce_whisper_dims dims{};
    bool loaded = false;
    DevBuf tables, logspec, clipmax, mel_tm, mel_start, mel_stage, w_bf16, w_f32, pos;
    bool mel_windowed = false;             // the last pce_logmel_run_at: windows start at mel_start[clip]
    int64_t stem_tiles_c1 = 0, stem_tiles_c2 = 0;     // row tiles the batch of the last log-mel run leaves out in conv1 / conv2, all clips together (0: the stem
                                                      // runs its two full launches, with no description and no fill)
    DevBuf stem_skip, stem_rep;            // int2 [2][n_clips_mel]: the row tiles conv1 | conv2 leave out per clip (k_logmel_norm writes them with the image);
                                           // float [clips][d]: conv2's accumulators of the repeated row (GemmSkip, k_stem_fill)
    DevBuf c1_out, resid, resid16, ln_out, qkv, vt, attn, hidden, final_out, enc_tab, delta, delta2;
    size_t vt_elems_zeroed = 0;
    std::vector<int> al_tab_host, al_tok_host, al_heads_host;     // what d_tab / d_tokens / d_heads hold (pce_whisper_align_run)
    // the padded images (one zero row before and after every clip's frames) are cleared when they are (re)allocated or their row width
    // changes, not per run: the kernels that fill them write every interior row and never a pad row (c1_out alone was a 1.2 GB memset per encode)
    size_t mel_tm_zero_cap = 0, c1_zero_cap = 0, dvt_zero_cap = 0; int mel_tm_zero_nm = 0, c1_zero_d = 0;
    // text decoder
    pce_whisper_text_dims tdims{};
    bool dec_loaded = false;
    DevBuf dw_bf16, dw_f32, d_tok_emb, d_pos_emb;
    DevBuf d_tab, d_tokens, d_resid, d_ln, d_qk, d_vt, d_attn, d_q, d_hidden, d_enc_bf16, d_aw, d_cost, d_trace, d_pi, d_pj, d_pl, d_heads;
    int enc_bf16_clips = -1;             // d_enc_bf16 holds the op_t copy of final_out for this many clips (written by the encoder's last LayerNorm)
    // free-running decoding: tied output projection in op_t (rows padded to 128), cross K / V of every layer, last-position buffers
    DevBuf g_emb_bf16, g_xk, g_xvt, g_last, g_lastln, g_logits, g_mask, g_next, g_keys;
    DevBuf g_lang;                   // pce_whisper_detect_language: probabilities [clips][n_lang] fp32 | token ids [clips]
    DevBuf g_wkT, g_qp, g_upart, g_mlpart;   // cross-attention from the encoder output (pce_xattn.inc): Wk^T of every layer, Q' hi | lo, the splits' partial U and (m, l)
    int g_keys_n = 0;                // sampling keys of the encoded batch (pce_whisper_sample_keys); 0: the batch position is the key
    int g_xkv_clips = -1;            // clips the cross K / V cache was computed for (-1: stale)
    // self-attention K / V of the sequences decoded so far: K rows [layer][clip][T_cap][d], V^T [layer][clip][d][512]
    DevBuf g_sv;                      // V rows [layer][clip][T_cap][d] of the incremental steps' self-attention (k_self_attn1w); g_svt = the prefix kernels' V^T image
    DevBuf g_sk, g_svt, g_c_resid, g_c_ln, g_c_qkv, g_c_attn, g_c_q, g_c_hidden, g_c_tab, g_loop;
    std::vector<int> g_cache_tok;     // host copy of the cached prefixes [clip][T_cap]
    int g_cache_len = -1, g_cache_n = -1;   // g_cache_len: < 0 = nothing cached (new encoded batch); per-sequence lengths in g_cache_lens
    std::vector<int> g_cache_lens;
    struct DLayer { size_t ln1_w, ln1_b, qkv_w, qkv_b, out_w, out_b, lnx_w, lnx_b, xq_w, xq_b, xkv_w, xkv_b, xout_w, xout_b,
                    ln2_w, ln2_b, m1_w, m1_b, m2_w, m2_b; };
    std::vector<DLayer> dlayers;
    size_t dln_w = 0, dln_b = 0;
    int al_n = -1, al_Nmax = 0, al_Fpad = 0, al_Mmax = 0;
    std::vector<int> al_rows, al_cols;
    // asynchronous fetch of every clip's DTW path (pce_whisper_align_paths_enqueue / _wait): pinned staging, two batches in flight
    struct PathSlot { void *host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool armed = false; int n = 0, stride = 0; } al_slot[2];
    bool lds_opted_in = false;        // lds_optins has run
    MelTables mt{};
    int mel_nmels = 0;
    int32_t n_clips_mel = -1, n_clips_enc = -1, enc_tab_clips = -1;
    // break-prediction token classifier (BertForTokenClassification)
    struct Bert {
        pce_bert_dims dims{};
        bool loaded = false;
        DevBuf w_bf16, w_f32, word, pos, type0;
        DevBuf tab, tokens, resid, ln, qk, vt, attn, hidden, logits;
        struct Layer { size_t qkv_w, qkv_b, out_w, out_b, ln1_w, ln1_b, m1_w, m1_b, m2_w, m2_b, ln2_w, ln2_b; };
        std::vector<Layer> layers;
        size_t lne_w = 0, lne_b = 0, cls_w = 0, cls_b = 0;
        int n_seq = -1, T_pad = 0;
        std::vector<int> lens;
    } bert;
    // wav2vec2 / MMS CTC acoustic model (pce_w2v.inc): weights, the images of one chunk of windows, the packed emissions of the batch
    struct W2v {
        pce_w2v_dims dims{};
        bool loaded = false;
        DevBuf w16, w32;
        struct Conv { size_t w = 0, b = 0, g = 0, beta = 0; bool has_b = false, has_ln = false; } conv[8];
        struct Layer { size_t qkv_w, qkv_b, out_w, out_b, ln1_w, ln1_b, m1_w, m1_b, m2_w, m2_b, ln2_w, ln2_b; };
        std::vector<Layer> layers;
        size_t fp_ln_w = 0, fp_ln_b = 0, proj_w = 0, proj_b = 0, pos_w = 0, pos_b = 0, enc_ln_w = 0, enc_ln_b = 0, lm_w = 0, lm_b = 0;
        int Vp = 0;                         // lm_head's columns, padded to whole GEMM tiles
        DevBuf img[2], part, ss, wintab, tailtab, atab, fpln, h0, h, ln, qk, vt, attn, hidden, logits, em;
        std::vector<int64_t> row_start;     // first row of clip q in em
        std::vector<int32_t> n_frames;
        int n_cols = 0, n_clips = -1;       // n_clips < 0: no run yet
    } w2v;
    // offsets (elements) into w_bf16 / w_f32
    struct Layer { size_t ln1_w, ln1_b, qkv_w, qkv_b, out_w, out_b, ln2_w, ln2_b, m1_w, m1_b, m2_w, m2_b; };
    size_t c1_w = 0, c1_b = 0, c2_w = 0, c2_b = 0, lnp_w = 0, lnp_b = 0;
    std::vector<Layer> layers;
};

WhisperState *ws_of(pce_ctx *c)
{
    if (!c->whisper_slot[PCE_OP_INDEX]) c->whisper_slot[PCE_OP_INDEX] = new WhisperState();
    return static_cast<WhisperState *>(c->whisper_slot[PCE_OP_INDEX]);
}

int mel_setup(pce_ctx *c, WhisperState *w, int n_mels)
{
    if (w->mel_nmels == n_mels) return PCE_OK;
    std::vector<float> dense; mel_filterbank(n_mels, dense);
    std::vector<int> lo((size_t)n_mels), cnt((size_t)n_mels), off((size_t)n_mels);
    std::vector<float> packed;
    for (int i = 0; i < n_mels; i++) {
        int a = 0, b = W_BINS;
        while (a < W_BINS && dense[(size_t)i * W_BINS + a] == 0.f) a++;
        while (b > a && dense[(size_t)i * W_BINS + b - 1] == 0.f) b--;
        lo[(size_t)i] = a; cnt[(size_t)i] = b - a; off[(size_t)i] = (int)packed.size();
        for (int k = a; k < b; k++) packed.push_back(dense[(size_t)i * W_BINS + k]);
    }
    std::vector<float> w16(32), w25(50), w400(800), win(W_NFFT);
    for (int m = 0; m < 16; m++) { w16[2 * (size_t)m] = (float)std::cos(2 * W_PI * m / 16); w16[2 * (size_t)m + 1] = (float)-std::sin(2 * W_PI * m / 16); }
    for (int m = 0; m < 25; m++) { w25[2 * (size_t)m] = (float)std::cos(2 * W_PI * m / 25); w25[2 * (size_t)m + 1] = (float)-std::sin(2 * W_PI * m / 25); }
    for (int n2 = 0; n2 < 25; n2++)
        for (int k1 = 0; k1 < 16; k1++) {
            const double a = 2 * W_PI * (n2 * k1) / 400.0;
            w400[2 * (size_t)(n2 * 16 + k1)] = (float)std::cos(a); w400[2 * (size_t)(n2 * 16 + k1) + 1] = (float)-std::sin(a);
        }
    for (int n = 0; n < W_NFFT; n++) win[(size_t)n] = (float)(0.5 - 0.5 * std::cos(2 * W_PI * n / W_NFFT));
    // one buffer: [w16 | w400 | w25 | window | lo | cnt | off | packed]
    const size_t bytes = sizeof(float) * (32 + 800 + 50 + W_NFFT + packed.size()) + sizeof(int) * 3 * (size_t)n_mels + 64;
    PCE_HIP(c, w->tables.reserve(bytes));
    char *d = w->tables.as<char>(); size_t o = 0;
    auto put = [&](const void *src, size_t n) -> const void * {
        (void)hipMemcpyAsync(d + o, src, n, hipMemcpyHostToDevice, c->stream);
        const void *p = d + o; o += (n + 15) & ~(size_t)15; return p;
    };
    w->mt.w16 = (const float2 *)put(w16.data(), sizeof(float) * 32);
    w->mt.w400 = (const float2 *)put(w400.data(), sizeof(float) * 800);
    w->mt.w25 = (const float2 *)put(w25.data(), sizeof(float) * 50);
    w->mt.window = (const float *)put(win.data(), sizeof(float) * W_NFFT);
    w->mt.mel_lo = (const int *)put(lo.data(), sizeof(int) * (size_t)n_mels);
    w->mt.mel_n = (const int *)put(cnt.data(), sizeof(int) * (size_t)n_mels);
    w->mt.mel_off = (const int *)put(off.data(), sizeof(int) * (size_t)n_mels);
    w->mt.mel_w = (const float *)put(packed.data(), sizeof(float) * packed.size());
    w->mt.mel_total = (int)packed.size();
    if (packed.size() > (size_t)LM_MELW) return pce_fail(c, PCE_E_LIMIT, "%zu packed mel weights (the kernel holds %d)", packed.size(), LM_MELW);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    w->mel_nmels = n_mels;
    return PCE_OK;
}

// Does every byte offset k_gemm_flat forms stay below 2^32?  rows_pad = the rows its padded tile list reaches.
static bool gemm_flat_offsets_fit(int64_t M, int64_t N, int64_t K, int64_t ldc, int64_t S, int64_t vt_sp)
{
    const int64_t tiles_m = (M + F_T - 1) / F_T, rows_pad = ((tiles_m + 15) / 16) * 16 * F_T, lim = 1ll << 32;
    if (rows_pad * K * 2 >= lim || N * K * 2 >= lim) return false;
    if (S > 0) return (rows_pad / S + 2) * N * vt_sp * 2 < lim;           // V^T image: one clip block per S rows (+ the clip a tile may spill into)
    return rows_pad * ldc * 2 < lim;
}

// Persistent 256 x 256 GEMM (pce_gemm256.inc) for the big projections: A dense [M][K], C op_t.  Returns false when the shape does not fit
// (the caller then takes the tiled kernels).
template <int EPI>
bool launch_gemm_flat(pce_ctx *c, const op_t *A, const op_t *B, const float *bias, op_t *C, int M, int N, int K, int ldc, int S = 1, int vt_sp = 0,
                      int prof_id = PCE_K_GEMM_FLAT, op_t *C2 = nullptr, int vt_n0 = 0, const op_t *R = nullptr)
{
    // 32-bit byte offsets: the kernel addresses the row tiles up to the PADDED tile count (16 row tiles per supertile); rows past M must
    // fall outside the buffer resources (loads read zeros, stores are dropped), which only holds while their offsets do not wrap
    constexpr bool HAS_VT = EPI == FEPI_VT || EPI == FEPI_SPLIT, HAS_RM = EPI != FEPI_VT;
    // (no lower bound on M: which kernel computes a projection must follow from the MODEL's dims alone, never from the batch size -- a clip's
    // results are compared across batch compositions and rank counts, tests/test_gpu_world2.py)
    if (!c->gemm_flat || N % F_T || K % F_K || M < 1 || N > F_N_MAX || (HAS_VT && (S % 4 || S < F_T))) return false;
    if (EPI == FEPI_SPLIT && (!C2 || vt_n0 <= 0 || vt_n0 >= N || vt_n0 % F_T)) return false;
    if (EPI == FEPI_RESID && !R) return false;
    if (HAS_RM && !gemm_flat_offsets_fit(M, N, K, ldc, 0, 0)) return false;
    if (HAS_VT && !gemm_flat_offsets_fit(M, N - vt_n0, K, 0, S, vt_sp)) return false;
    FArgs P{};
    P.A = A; P.B = B; P.bias = bias; P.C = C; P.M = M; P.N = N; P.K = K; P.ldc = ldc; P.S = S; P.vt_sp = vt_sp; P.C2 = C2; P.vt_n0 = vt_n0; P.R = R;
    const int tiles_n = N / F_T;
    P.sn = 1;
    for (int cand : {4, 3, 2}) if (tiles_n % cand == 0) { P.sn = cand; break; }
    const int tiles_m = (M + F_T - 1) / F_T;
    int sm_want = 16;
    P.stagger = 20000;
    // per-shape walks from the sweeps of round 5 (profiles/r05/flat_walk.txt, flat_shape_walk_ab.txt: same box, alternating): a 3-tile-wide product
    // of short K (the attention out-projection) column by column in 8-row supertiles (436 -> 422 us), 6 tiles across (cross K|V) the whole width
    // at once (835 -> 817 us); qkv (9 across), fc1 (12) and fc2 (3 across, K = 3072) stay on the default -- the whole width for fc1 gained 5 us
    // there and cost fc2, which reads what fc1 wrote, 22
    if (tiles_n == 3 && K <= 1024) { P.sn = 1; sm_want = 8; }
    else if (tiles_n == 6) P.sn = tiles_n;
    P.sm = tiles_m < sm_want ? tiles_m : sm_want;                           // (a short batch: no padding row tiles in the walk)
    const int lds = F_RING_BYTES + N * (int)sizeof(float);              // (N <= F_N_MAX: within what lds_optins allows)
    const int grid = ((c->cu_count > 0 ? c->cu_count : 256) / 8) * 8;
    KernelTimer kt(c, prof_id, nullptr, 2.0 * M * (double)N * K);
    hipLaunchKernelGGL((k_gemm_flat<EPI>), dim3((unsigned)grid), dim3(F_THREADS), lds, c->stream, P);
    return true;
}

// ---- the tiled / few-row GEMM kernels behind launch_gemm: which one runs (gemm_choose), what each can compute (gemm_fits), one launcher each
enum GemmKernel { GK_AUTO = 0, GK_SKINNY = 1, GK_WIDE = 2, GK_128 = 3, GK_128_DEEP = 4 };      // (pce_selftest_gemm_tiled's selector)
struct GemmShape { int M, N, K; int64_t lda; int batch; int v_col0; };
// The shapes a kernel computes exactly.  Every tiled kernel stores whole 128-column tiles (N % 128) and walks K in whole steps: k_gemm_bf16's
// nk = K / 64 and k_gemm_wide's K / 32 would drop a tail.  The few-row kernel: one batch entry, 256-deep K chunks, 16-byte A rows.
template <int EPI> static bool gemm_fits(int kind, const GemmShape &s)
{
    switch (kind) {
    case GK_SKINNY:
        return (EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_RESID_F32) && s.batch == 1 && s.M <= 1024 && s.N <= 4096 && s.N % S_BN == 0 &&
               s.K % S_KC == 0 && s.lda % 8 == 0;
    case GK_WIDE: return s.N % W_BN == 0 && s.K % W_BK == 0 && (EPI != EPI_QKV || s.v_col0 % W_BN == 0);
    case GK_128: case GK_128_DEEP: return s.N % G_BN == 0 && s.K % G_BK == 0 && (EPI != EPI_QKV || s.v_col0 % G_BN == 0);
    default: return false;
    }
}
// The product's rule
template <int EPI> static int gemm_choose(const pce_ctx *c, const GemmShape &s)
{
    // a few rows x a few thousand columns (the projections of an incremental decoding step): the latency-shaped kernel
    // Only where the caller asks for it (the incremental decoding step): which kernel runs must not follow from the BATCH SIZE of a leg whose
    // results are compared across batch sizes -- the few-row kernel and the tiled ones sum identically (bit-identical bias and fp32
    // accumulate epilogues, tests/test_gpu_kernels.py) but the compiler schedules the inlined GELU differently in the two, and on fp16
    // operands 6e-5 of the GELU outputs then round to the neighbouring value (tests/test_gpu_whisper.py::test_c3_batch_of_256_is_clip_independent)
    if (c->gemm_skinny && c->gemm_few_rows && gemm_fits<EPI>(GK_SKINNY, s)) return GK_SKINNY;
    // (chosen by N and K alone: the two tiled kernels round a GELU epilogue differently in a few outputs per 10^5, so the choice must not follow from M)
    // (the vocabulary logits of a decoding step -- a few hundred rows x 51 968 columns, fp32 out -- take the deep-ring 128 x 128 kernel below: 55 against 68 us;
    //  plain fp32 sums: the tiled kernels add the same products in the same order)
    if (gemm_fits<EPI>(GK_WIDE, s) && s.N >= 1536 && !(EPI == EPI_F32 && (int64_t)s.M * s.batch <= 1024))     // wide outputs (QKV, fc1; from N = 1536 so
        return GK_WIDE;                                                                                          // that the tiny model exercises it in the tests)
    if ((int64_t)s.M * s.batch <= 1024 && s.K >= 4 * G_BK) return GK_128_DEEP;     // a few rows (incremental decoding step): few workgroups, each alone on its CU
    return GK_128;
}
template <int EPI>
static void launch_gemm_kernel(pce_ctx *c, int kind, const op_t *A, int64_t lda, int64_t a_batch, const op_t *B, int M, int N, int K, const float *bias,
                               void *C, int64_t ldc, int64_t c_batch, int batch, const float *pos, int pos_T, int v_col0, int vt_sp,
                               const GemmSkip &skip = GemmSkip{nullptr, nullptr, 0, 0})       // only the GK_128 kernel takes one (pce_whisper_encode_run asks first)
{
    if constexpr (EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_RESID_F32) {
        if (kind == GK_SKINNY) {
            KernelTimer kt(c, PCE_K_GEMM_SKINNY, nullptr, 2.0 * M * (double)N * K);
            hipLaunchKernelGGL((k_gemm_skinny<EPI>), dim3((unsigned)(N / S_BN), (unsigned)div_up(M, S_BM)), dim3(S_THREADS), S_LDS, c->stream,
                               A, lda, B, M, N, K, bias, C, ldc);
            return;
        }
    }
    if (kind == GK_WIDE) {
        const int wt = N / W_BN;
        int wsn = 1;
        for (int cand : {4, 3, 2}) if (wt % cand == 0) { wsn = cand; break; }
        const int wsm = 16;
        dim3 wgrid((unsigned)wt, (unsigned)(div_up(M, G_BM * wsm) * wsm), (unsigned)batch);
        KernelTimer kt(c, PCE_K_GEMM_WIDE, nullptr, 2.0 * M * (double)N * K * batch);
        hipLaunchKernelGGL((k_gemm_wide<EPI>), wgrid, dim3(G_THREADS), 0, c->stream, A, lda, a_batch, B, M, N, K, bias, C, ldc, c_batch, pos, pos_T,
                           v_col0, vt_sp, wsn, wsm);
        return;
    }
    const int tiles_n = N / G_BN;
    int sn = 1;
    for (int cand : {8, 6, 4, 3, 2}) if (tiles_n % cand == 0) { sn = cand; break; }        // supertile width (divides the N tiles)
    const int sm = 16;                                     // 16 x sn measured best by a hair (645-656 TFLOP/s over 4..16 x 2..8)
    dim3 grid((unsigned)tiles_n, (unsigned)(div_up(M, G_BM * sm) * sm), (unsigned)batch);
    KernelTimer kt(c, PCE_K_GEMM128, nullptr, 2.0 * ((double)M * batch - (double)skip.skipped_rows) * N * K);      // the rows that are multiplied
    if (kind == GK_128_DEEP)
        hipLaunchKernelGGL((k_gemm_bf16<EPI, 4>), grid, dim3(G_THREADS), 0, c->stream, A, lda, a_batch, B, M, N, K, bias, C, ldc, c_batch, pos, pos_T,
                           v_col0, vt_sp, sn, sm, GemmSkip{nullptr, nullptr, 0, 0});
    else
        hipLaunchKernelGGL((k_gemm_bf16<EPI>), grid, dim3(G_THREADS), 0, c->stream, A, lda, a_batch, B, M, N, K, bias, C, ldc, c_batch, pos, pos_T,
                           v_col0, vt_sp, sn, sm, skip);
}
template <int EPI>
void launch_gemm(pce_ctx *c, const op_t *A, int64_t lda, int64_t a_batch, const op_t *B, int M, int N, int K, const float *bias,
                 void *C, int64_t ldc, int64_t c_batch, int batch, const float *pos = nullptr, int pos_T = 1, int v_col0 = 0,
                 int vt_sp = AT_SP, const GemmSkip *skip = nullptr)
{
    const int kind = gemm_choose<EPI>(c, GemmShape{M, N, K, lda, batch, v_col0});
    if (skip && kind == GK_128) launch_gemm_kernel<EPI>(c, kind, A, lda, a_batch, B, M, N, K, bias, C, ldc, c_batch, batch, pos, pos_T, v_col0, vt_sp, *skip);
    else launch_gemm_kernel<EPI>(c, kind, A, lda, a_batch, B, M, N, K, bias, C, ldc, c_batch, batch, pos, pos_T, v_col0, vt_sp);
}

// ---- LayerNorm launches: four rows (waves) per workgroup, the register form by width (k_layernorm); d <= LN_D_MAX, d % 4 == 0 (the loaders)
template <class OUT>
static void launch_layernorm(pce_ctx *c, const float *x, const float *w, const float *b, int64_t rows, int d, OUT *out, float eps = 1e-5f,
                             float *out2 = nullptr, int round_in16 = 0, op_t *in16_out = nullptr)
{
    const dim3 grid((unsigned)div_up(rows, 4)), block(256);
    if (d <= 1280) hipLaunchKernelGGL((k_layernorm<OUT, 5>), grid, block, 0, c->stream, x, w, b, rows, d, out, eps, out2, round_in16, in16_out);
    else hipLaunchKernelGGL((k_layernorm<OUT, 8>), grid, block, 0, c->stream, x, w, b, rows, d, out, eps, out2, round_in16, in16_out);
}
template <class OUT, class RIN, class ROUT>
static void launch_add_layernorm(pce_ctx *c, const RIN *resid_in, ROUT *resid_out, const op_t *delta, const op_t *delta2, int write_resid, const float *w,
                                 const float *b, int64_t rows, int d, OUT *out, float eps, op_t *out_bf16)
{
    const dim3 grid((unsigned)div_up(rows, 4)), block(256);
    if (d <= 1280)
        hipLaunchKernelGGL((k_add_layernorm<OUT, RIN, ROUT, 5>), grid, block, 0, c->stream, resid_in, resid_out, delta, delta2, write_resid, w, b, rows, d, out, eps, out_bf16);
    else
        hipLaunchKernelGGL((k_add_layernorm<OUT, RIN, ROUT, 8>), grid, block, 0, c->stream, resid_in, resid_out, delta, delta2, write_resid, w, b, rows, d, out, eps, out_bf16);
}

template <class OUT>
static void launch_add_layernorm0(pce_ctx *c, const op_t *x, const float *w, const float *b, int64_t rows, int d, OUT *out, float eps, op_t *out_bf16)
{
    const dim3 grid((unsigned)div_up(rows, 4 * LN0_ROWS)), block(256);
    if (d <= 1280) hipLaunchKernelGGL((k_add_layernorm0<OUT, 5>), grid, block, 0, c->stream, x, w, b, rows, d, out, eps, out_bf16);
    else hipLaunchKernelGGL((k_add_layernorm0<OUT, 8>), grid, block, 0, c->stream, x, w, b, rows, d, out, eps, out_bf16);
}

// ---- the encoder-output cross-attention of a decoding step (pce_xattn.inc), as the product and pce_selftest_xattn launch it --------------------
// The widths it is built for, with 64-wide heads (at most 20: large-v3 / turbo)
static bool xa_has_form(int d, int heads)
{
    return heads * 64 == d && (d == 128 || d == 256 || d == 384 || d == 512 || d == 768 || d == 1024 || d == 1280);
}
// workgroups per clip (two per CU): ONLY the work distribution follows the batch size -- the frames are always cut into the same XA_LEAVES ranges
// and merged in the same order (pce_xattn.inc), so a clip's bits do not depend on what it is batched with.  wpc = 1 | 2 | 4 overrides (tests)
static int xa_split(int n, int wpc) { return (wpc == 1 || wpc == 2 || wpc == 4) ? wpc : n >= 512 ? 1 : n >= 256 ? 2 : 4; }
// The choices of one width: ring slots; the pair form (a workgroup that owns both leaves of a pair, nsplit <= 2, merges them in registers and
// writes pair nodes) up to d = 768 -- d = 1024 has no registers for the waiting leaf (194 + 64) and always writes leaves; d = 1280 (20 heads): two
// 16-row tiles of heads, 8 waves per workgroup (136 KB of LDS: one workgroup per CU)
template <int D> struct XaWidth {
    static constexpr int NSLOT = (D == 512 || D == 768 || D == 1024) ? 2 : 3, WV = xa_waves(D), RT = D > 1024 ? 2 : 1;
    static constexpr bool PAIRS = D <= 768;
    static constexpr size_t LDS = xa_lds(D, NSLOT);
};
// One layer's operands besides XaArgs: k_xq_fused's (LayerNorm, query projection, Wk^T; it writes Q' to qp_hi | qp_lo) and k_uv_absorb's (Wv, bv, out)
struct XaLayer {
    const float *resid, *ln_w, *ln_b, *bq, *bv;
    const op_t *wq, *wkT, *wv;
    op_t *qp_hi, *qp_lo, *out; int64_t out_ld;
};
// k_xq_fused -> k_xattn_absorbed -> k_uv_absorb for n clips
template <int D>
static void xattn_launch_d(pce_ctx *c, int n, XaArgs a, const XaLayer &y)
{
    using W = XaWidth<D>;
    a.qp_hi = y.qp_hi; a.qp_lo = y.qp_lo;
    const dim3 hgrid((unsigned)a.heads, (unsigned)div_up(n, 16)), grid((unsigned)(n * a.nsplit)), block(64 * (unsigned)W::WV);
    hipLaunchKernelGGL(k_xq_fused<D>, hgrid, dim3(256), 0, c->stream, y.resid, y.ln_w, y.ln_b, y.wq, y.bq, y.wkT, n, 0.125f * 1.4426950408889634f, a.skip,
                       y.qp_hi, y.qp_lo, a.rows);
    auto uv = [&](auto kern) {
        hipLaunchKernelGGL(kern, hgrid, dim3(256), 0, c->stream, a.u_part, a.ml_part, y.wv, y.bv, n, a.skip, y.out, y.out_ld, a.rows);
    };
    if constexpr (W::PAIRS) {
        if (a.nsplit <= XA_LEAVES / 2) {
            hipLaunchKernelGGL((k_xattn_absorbed<D, W::NSLOT, true, W::WV, W::RT>), grid, block, W::LDS, c->stream, a);
            uv(k_uv_absorb<D, true>);
            return;
        }
    }
    hipLaunchKernelGGL((k_xattn_absorbed<D, W::NSLOT, false, W::WV, W::RT>), grid, block, W::LDS, c->stream, a);
    uv(k_uv_absorb<D, false>);
}
static void xattn_launch(pce_ctx *c, int d, int n, const XaArgs &a, const XaLayer &y)       // (xa_has_form(d, a.heads))
{
    switch (d) {
    case 128: xattn_launch_d<128>(c, n, a, y); break;
    case 256: xattn_launch_d<256>(c, n, a, y); break;
    case 384: xattn_launch_d<384>(c, n, a, y); break;
    case 512: xattn_launch_d<512>(c, n, a, y); break;
    case 768: xattn_launch_d<768>(c, n, a, y); break;
    case 1024: xattn_launch_d<1024>(c, n, a, y); break;
    default: xattn_launch_d<1280>(c, n, a, y); break;
    }
}

// Dynamic-LDS opt-ins (hipFuncSetAttribute) of every kernel of this operand build that launches with more LDS than the default allows: once per
// WhisperState (the attribute is per device: the context's), before the first launch that needs one -- from the *_load entry points and the
// self-tests.  A failure is an error: which kernel computes a product follows from the shapes alone.
template <int D> static hipError_t xattn_optin()
{
    using W = XaWidth<D>;
    if constexpr (W::PAIRS) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_xattn_absorbed<D, W::NSLOT, true, W::WV, W::RT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)W::LDS);
        if (e != hipSuccess) return e;
    }
    return hipFuncSetAttribute((const void *)k_xattn_absorbed<D, W::NSLOT, false, W::WV, W::RT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)W::LDS);
}
static int lds_optins(pce_ctx *c, WhisperState *w)
{
    if (w->lds_opted_in) return PCE_OK;
    const hipFuncAttribute A = hipFuncAttributeMaxDynamicSharedMemorySize;
    const int flat = F_RING_BYTES + F_N_MAX * (int)sizeof(float);             // the ring + the widest bias vector launch_gemm_flat admits
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_gemm_flat<FEPI_BF16>, A, flat));
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_gemm_flat<FEPI_GELU>, A, flat));
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_gemm_flat<FEPI_VT>, A, flat));
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_gemm_flat<FEPI_SPLIT>, A, flat));
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_gemm_flat<FEPI_RESID>, A, flat));
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_gemm_skinny<EPI_BF16>, A, S_LDS));
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_gemm_skinny<EPI_GELU_BF16>, A, S_LDS));
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_gemm_skinny<EPI_RESID_F32>, A, S_LDS));
    PCE_HIP(c, hipFuncSetAttribute((const void *)k_cross_attn1w, A, 16 * 1600 * 4));   // 16 waves' score slices: the largest head group
    PCE_HIP(c, xattn_optin<128>()); PCE_HIP(c, xattn_optin<256>()); PCE_HIP(c, xattn_optin<384>()); PCE_HIP(c, xattn_optin<512>());
    PCE_HIP(c, xattn_optin<768>()); PCE_HIP(c, xattn_optin<1024>()); PCE_HIP(c, xattn_optin<1280>());
    w->lds_opted_in = true;
    return PCE_OK;
}

} // namespace

void pce_whisper_free(pce_ctx *c)
{
    if (!c->whisper_slot[PCE_OP_INDEX]) return;
    WhisperState *w = static_cast<WhisperState *>(c->whisper_slot[PCE_OP_INDEX]);
    for (auto &ps : w->al_slot) {
        if (ps.host) (void)hipHostFree(ps.host);
        if (ps.ev) (void)hipEventDestroy(ps.ev);
    }
    delete w;
    c->whisper_slot[PCE_OP_INDEX] = nullptr;
}

extern "C" {

static int logmel_run_impl(pce_ctx *c, int32_t n_mels, const int64_t *start_frames);
int pce_logmel_run(pce_ctx *c, int32_t n_mels) { return logmel_run_impl(c, n_mels, nullptr); }
int pce_logmel_run_at(pce_ctx *c, int32_t n_mels, const int64_t *start_frames)
{
    if (!start_frames) return PCE_E_INVALID;
    return logmel_run_impl(c, n_mels, start_frames);
}
static int logmel_run_impl(pce_ctx *c, int32_t n_mels, const int64_t *start_frames)
{
    if (!c) return PCE_E_INVALID;
    if (!c->d_pcm) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    if (c->rate != 16000) return pce_fail(c, PCE_E_INVALID, "log-mel needs 16 kHz audio (got %d Hz): resample on the host first", c->rate);
    if (n_mels <= 0 || n_mels > 128) return pce_fail(c, PCE_E_INVALID, "n_mels %d out of range", n_mels);
    PCE_HIP(c, hipSetDevice(c->device));
    WhisperState *w = ws_of(c);
    int rc = mel_setup(c, w, n_mels);
    if (rc) return rc;
    const int32_t n = c->n_clips;
    const size_t tm_elems = (size_t)n * (W_FRAMES + 2) * (size_t)n_mels + 512;
    PCE_HIP(c, w->logspec.reserve(sizeof(float) * (size_t)n * (size_t)n_mels * W_FRAMES));
    PCE_HIP(c, w->clipmax.reserve(sizeof(unsigned int) * (size_t)n));
    PCE_HIP(c, w->mel_tm.reserve(sizeof(op_t) * tm_elems));
    PCE_HIP(c, w->stem_skip.reserve(sizeof(int2) * 2 * (size_t)(n > 0 ? n : 1)));
    w->stem_tiles_c1 = w->stem_tiles_c2 = 0;
    for (int32_t i = 0; i < n; i++) {      // what k_logmel_norm will write per clip, summed from the host's copy of the same lengths and starts
        const int64_t full = c->clip_off[(size_t)i + 1] - c->clip_off[(size_t)i];
        const int s = stem_first_skipped_tile(start_frames ? full : std::min<int64_t>(full, W_SAMPLES), start_frames ? start_frames[i] : 0);
        if (s < ST_C2_LAST) { w->stem_tiles_c2 += ST_C2_LAST - s; w->stem_tiles_c1 += ST_C1_KEEP - 2 * s; }
    }
    PCE_HIP(c, hipMemsetAsync(w->clipmax.p, 0, sizeof(unsigned int) * (size_t)n, c->stream));
    if (w->mel_tm.cap != w->mel_tm_zero_cap || w->mel_tm_zero_nm != n_mels) {
        PCE_HIP(c, hipMemsetAsync(w->mel_tm.p, 0, w->mel_tm.cap, c->stream));
        w->mel_tm_zero_cap = w->mel_tm.cap; w->mel_tm_zero_nm = n_mels;
    }
    constexpr int LM_G = 16;
    const size_t lm_lds = sizeof(float) * 4 * (size_t)n_mels * (LM_G + 1);
    const int64_t *d_start = nullptr;
    if (start_frames) {
        int64_t longest = 0;
        for (int32_t i = 0; i < n; i++) {
            const int64_t len = c->clip_off[(size_t)i + 1] - c->clip_off[(size_t)i];
            if (start_frames[i] < 0 || start_frames[i] * W_HOP > len) return pce_fail(c, PCE_E_INVALID, "clip %d: window start %lld frames is past the audio", i, (long long)start_frames[i]);
            longest = std::max(longest, len);
        }
        PCE_HIP(c, w->mel_start.reserve(sizeof(int64_t) * (size_t)(n > 0 ? n : 1)));
        PCE_HIP(c, hipMemcpyAsync(w->mel_start.p, start_frames, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        PCE_HIP(c, hipStreamSynchronize(c->stream));
        d_start = w->mel_start.as<int64_t>();
        if (n > 0) {       // the clamp of log_mel_spectrogram uses the maximum over the whole recording
            const int64_t scan_frames = (longest + W_NFFT / 2) / W_HOP + 1;
            hipLaunchKernelGGL(k_logmel_frames<LM_G>, dim3((unsigned)std::min<int64_t>(div_up(scan_frames, 4 * LM_G), 4096), (unsigned)n), dim3(256), lm_lds, c->stream, c->d_pcm,
                               c->d_clip_off.as<int64_t>(), (int)n_mels, w->mt, w->logspec.as<float>(), w->clipmax.as<unsigned int>(), d_start, 1);
        }
    }
    {
        KernelTimer t(c, PCE_K_LOGMEL);
        // (16 frames per store group: 1.16-1.18 ms per C3 step against 1.30 for one frame and 1.33 for four, same box; with the table loads hoisted)
        hipLaunchKernelGGL(k_logmel_frames<LM_G>, dim3((unsigned)div_up(W_FRAMES, 4 * LM_G), (unsigned)n), dim3(256), lm_lds, c->stream, c->d_pcm,
                           c->d_clip_off.as<int64_t>(), (int)n_mels, w->mt, w->logspec.as<float>(), w->clipmax.as<unsigned int>(), d_start, 0);
    }
    {
        KernelTimer t(c, PCE_K_LOGMEL_NORM);
        hipLaunchKernelGGL(k_logmel_norm, dim3(div_up(W_FRAMES, 64), div_up(n_mels, 64), (unsigned)n), dim3(256), 0, c->stream,
                           w->logspec.as<float>(), w->clipmax.as<unsigned int>(), (int)n_mels, c->d_clip_off.as<int64_t>(), d_start, 0, w->mel_tm.as<op_t>(), (float *)nullptr,
                           w->stem_skip.as<int2>(), w->stem_skip.as<int2>() + n);
    }
    PCE_HIP(c, hipGetLastError());
    w->n_clips_mel = n;
    w->mel_windowed = start_frames != nullptr;
    return PCE_OK;
}

int pce_logmel_fetch(pce_ctx *c, int32_t clip, float *out)
{
    if (!c || !out) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (w->n_clips_mel < 0) return pce_fail(c, PCE_E_STATE, "pce_logmel_fetch before pce_logmel_run");
    if (clip < 0 || clip >= w->n_clips_mel) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    const size_t per = (size_t)w->mel_nmels * W_FRAMES;
    // the float matrix of ONE clip, finished on its way out (the resident values are raw log10: see k_logmel_norm)
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_HIP(c, w->mel_stage.reserve(sizeof(float) * per + 64));
    hipLaunchKernelGGL(k_logmel_norm, dim3(div_up(W_FRAMES, 64), div_up(w->mel_nmels, 64), 1), dim3(256), 0, c->stream, w->logspec.as<float>(),
                       w->clipmax.as<unsigned int>(), (int)w->mel_nmels, c->d_clip_off.as<int64_t>(), w->mel_windowed ? w->mel_start.as<int64_t>() : (const int64_t *)nullptr,
                       (int)clip, (op_t *)nullptr, w->mel_stage.as<float>(), (int2 *)nullptr, (int2 *)nullptr);
    PCE_HIP(c, hipGetLastError());
    PCE_HIP(c, hipMemcpyAsync(out, w->mel_stage.p, sizeof(float) * per, hipMemcpyDeviceToHost, c->stream));
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

// the op_t time-major image of one clip as the last run left it (what the conv stem reads), copied out: nothing is launched, nothing written
int pce_selftest_logmel_image(pce_ctx *c, int32_t clip, uint16_t *out)
{
    if (!c || !out) return PCE_E_INVALID;
    WhisperState *w = ws_of(c);
    if (w->n_clips_mel < 0) return pce_fail(c, PCE_E_STATE, "pce_selftest_logmel_image before pce_logmel_run");
    if (clip < 0 || clip >= w->n_clips_mel) return pce_fail(c, PCE_E_INVALID, "clip out of range");
    static_assert(sizeof(op_t) == sizeof(uint16_t), "the image travels as 16-bit patterns");
    const size_t per = (size_t)(W_FRAMES + 2) * (size_t)w->mel_nmels;
    if (sizeof(op_t) * per * ((size_t)clip + 1) > w->mel_tm.cap) return pce_fail(c, PCE_E_STATE, "the last log-mel run did not finish: run it again");
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_HIP(c, hipMemcpyAsync(out, w->mel_tm.as<op_t>() + (size_t)clip * per, sizeof(op_t) * per, hipMemcpyDeviceToHost, c->stream));
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

int pce_whisper_load(pce_ctx *c, const pce_whisper_dims *dims, const float *weights, int64_t n_floats)
{
    if (!c || !dims || !weights) return PCE_E_INVALID;
    const int d = dims->n_state, L = dims->n_layer, nm = dims->n_mels;
    if (d <= 0 || d % 128 || dims->n_head * 64 != d || L <= 0 || dims->n_ctx != W_CTX || nm <= 0 || nm > 128 || (nm % 8))
        return pce_fail(c, PCE_E_LIMIT, "unsupported encoder dims (need n_state %% 128 == 0, head size 64, n_ctx 1500, n_mels %% 8 == 0)");
    if (d > LN_D_MAX) return pce_fail(c, PCE_E_LIMIT, "encoder with n_state %d: the LayerNorm kernels hold at most %d", d, LN_D_MAX);
    // pce_whisper_encode_run takes the persistent GEMM for every projection when n_state % 256 == 0; its fc1 (N = 4 n_state) must fit it too
    if (c->gemm_flat && d % F_T == 0 && 4 * d > F_N_MAX)
        return pce_fail(c, PCE_E_LIMIT, "encoder with n_state %d: the persistent GEMM's fc1 holds 4 n_state <= %d (PCE_GEMM_FLAT=0 at pce_create runs it on the "
                                        "tiled kernels)", d, F_N_MAX);
    const int64_t per_layer = 2LL * d + 4LL * d * d + 3LL * d + 2LL * d + 8LL * d * d + 5LL * d;
    const int64_t expect = (int64_t)d * nm * 3 + d + 3LL * d * d + d + L * per_layer + 2LL * d;
    if (n_floats != expect) return pce_fail(c, PCE_E_INVALID, "weight blob has %lld floats, expected %lld", (long long)n_floats, (long long)expect);
    PCE_HIP(c, hipSetDevice(c->device));
    WhisperState *w = ws_of(c);
    { const int rc = lds_optins(c, w); if (rc) return rc; }
    w->dims = *dims; w->loaded = false; w->layers.assign((size_t)L, {});
    // host repack: op_t-bound matrices (as fp32, converted on the device) and fp32 vectors
    std::vector<float> mats, vecs;
    auto add_vec = [&](const float *p, size_t n) { size_t o = vecs.size(); vecs.insert(vecs.end(), p, p + n); return o; };
    auto add_zero_vec = [&](size_t n) { size_t o = vecs.size(); vecs.insert(vecs.end(), n, 0.f); return o; };
    const float *p = weights;
    {   // conv1 [d][nm][3] -> [d][K1p] with k-major columns (k*nm + ci), zero padded to a multiple of 64
        const int K1 = 3 * nm, K1p = (int)div_up(K1, 64) * 64;
        w->c1_w = mats.size(); mats.resize(mats.size() + (size_t)d * K1p, 0.f);
        for (int co = 0; co < d; co++)
            for (int ci = 0; ci < nm; ci++)
                for (int k = 0; k < 3; k++) mats[w->c1_w + (size_t)co * K1p + (size_t)k * nm + ci] = p[((size_t)co * nm + ci) * 3 + k];
        p += (size_t)d * nm * 3;
        w->c1_b = add_vec(p, (size_t)d); p += d;
    }
    {   // conv2 [d][d][3] -> [d][3 d]
        w->c2_w = mats.size(); mats.resize(mats.size() + (size_t)d * 3 * d, 0.f);
        for (int co = 0; co < d; co++)
            for (int ci = 0; ci < d; ci++)
                for (int k = 0; k < 3; k++) mats[w->c2_w + (size_t)co * 3 * d + (size_t)k * d + ci] = p[((size_t)co * d + ci) * 3 + k];
        p += (size_t)d * d * 3;
        w->c2_b = add_vec(p, (size_t)d); p += d;
    }
    for (int l = 0; l < L; l++) {
        WhisperState::Layer &ly = w->layers[(size_t)l];
        ly.ln1_w = add_vec(p, (size_t)d); p += d; ly.ln1_b = add_vec(p, (size_t)d); p += d;
        // q.w q.b k.w v.w v.b -> fused [3d][d], bias [q.b | 0 | v.b]
        ly.qkv_w = mats.size(); mats.resize(mats.size() + (size_t)3 * d * d);
        const float *qw = p, *qb = p + (size_t)d * d, *kw = qb + d, *vw = kw + (size_t)d * d, *vb = vw + (size_t)d * d;
        std::copy(qw, qw + (size_t)d * d, mats.begin() + (ptrdiff_t)ly.qkv_w);
        std::copy(kw, kw + (size_t)d * d, mats.begin() + (ptrdiff_t)(ly.qkv_w + (size_t)d * d));
        std::copy(vw, vw + (size_t)d * d, mats.begin() + (ptrdiff_t)(ly.qkv_w + 2 * (size_t)d * d));
        ly.qkv_b = add_vec(qb, (size_t)d); add_zero_vec((size_t)d); add_vec(vb, (size_t)d);
        p = vb + d;
        ly.out_w = mats.size(); mats.insert(mats.end(), p, p + (size_t)d * d); p += (size_t)d * d;
        ly.out_b = add_vec(p, (size_t)d); p += d;
        ly.ln2_w = add_vec(p, (size_t)d); p += d; ly.ln2_b = add_vec(p, (size_t)d); p += d;
        ly.m1_w = mats.size(); mats.insert(mats.end(), p, p + (size_t)4 * d * d); p += (size_t)4 * d * d;
        ly.m1_b = add_vec(p, (size_t)4 * d); p += 4 * d;
        ly.m2_w = mats.size(); mats.insert(mats.end(), p, p + (size_t)4 * d * d); p += (size_t)4 * d * d;
        ly.m2_b = add_vec(p, (size_t)d); p += d;
    }
    w->lnp_w = add_vec(p, (size_t)d); p += d; w->lnp_b = add_vec(p, (size_t)d); p += d;
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
    PCE_HIP(c, tmp.reserve(sizeof(float) * mats.size()));
    PCE_HIP(c, w->w_bf16.reserve(sizeof(op_t) * mats.size() + 256));
    PCE_HIP(c, w->w_f32.reserve(sizeof(float) * vecs.size()));
    PCE_HIP(c, w->pos.reserve(sizeof(float) * pos.size()));
    PCE_HIP(c, hipMemcpyAsync(tmp.p, mats.data(), sizeof(float) * mats.size(), hipMemcpyHostToDevice, c->stream));
    PCE_HIP(c, hipMemcpyAsync(w->w_f32.p, vecs.data(), sizeof(float) * vecs.size(), hipMemcpyHostToDevice, c->stream));
    PCE_HIP(c, hipMemcpyAsync(w->pos.p, pos.data(), sizeof(float) * pos.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_f32_to_bf16, dim3((unsigned)div_up((int64_t)mats.size(), 256)), dim3(256), 0, c->stream, tmp.as<float>(),
                       w->w_bf16.as<op_t>(), (int64_t)mats.size());
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
        PCE_HIP(c, w->enc_tab.reserve(sizeof(int) * tab.size()));
        PCE_HIP(c, hipMemcpyAsync(w->enc_tab.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, c->stream));
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
    const bool stem_skip = c->stem_skip && w->stem_tiles_c2 > 0 && gemm_choose<EPI_GELU_BF16>(c, GemmShape{W_FRAMES, d, K1p, nm, n, 0}) == GK_128 &&
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
    const bool flat = c->gemm_flat && d % F_T == 0 && gemm_flat_offsets_fit(M, 4 * d, 4 * d, 4 * d, 0, 0) &&
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
    const bool fused = resid16 && c->resid_epilogue != 0, fused_out = fused && c->resid_epilogue == 1;
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
    for (int l = 0; l < L; l++) {
        const WhisperState::Layer &ly = w->layers[(size_t)l];
        if (!flat || l == 0) {
            KernelTimer kt(c, PCE_K_LAYERNORM);
            launch_layernorm<op_t>(c, w->resid.as<float>(), Wf + ly.ln1_w, Wf + ly.ln1_b, M, d, w->ln_out.as<op_t>(), 1e-5f, nullptr, resid16 ? 1 : 0,
                                   fused ? w->resid16.as<op_t>() : nullptr);
        }
        // Q | K go to the row-major [M][2d] buffer, V is written transposed per head: one launch sweeps the LayerNorm output once
        const bool done = flat && launch_gemm_flat<FEPI_SPLIT>(c, w->ln_out.as<op_t>(), Wb + ly.qkv_w, Wf + ly.qkv_b, w->qkv.as<op_t>(), (int)M, 3 * d, d, 2 * d,
                                                                W_CTX, AT_SP, PCE_K_GEMM_FLAT_QKV, w->vt.as<op_t>(), 2 * d);
        if (flat && !done) return pce_fail(c, PCE_E_LIMIT, "Q | K | V projection does not fit the 256 x 256 kernel");
        if (!done)
            launch_gemm<EPI_QKV>(c, w->ln_out.as<op_t>(), d, 0, Wb + ly.qkv_w, (int)M, 3 * d, d, Wf + ly.qkv_b, w->qkv.as<op_t>(), 2 * d, 0, 1,
                                 reinterpret_cast<const float *>(w->vt.as<op_t>()), W_CTX, 2 * d, AT_SP);
        const int *row0 = w->enc_tab.as<int>(), *len = row0 + n;
        launch_attention_rows(c, n, H, W_CTX, w->qkv.as<op_t>(), 2 * d, w->qkv.as<op_t>() + d, 2 * d, w->vt.as<op_t>(), AT_SP, row0, len, row0, len,
                              w->attn.as<op_t>(), 0, 4.0 * W_CTX * (double)W_CTX * d * n);
        if (flat) {
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
            continue;
        }
        launch_gemm<EPI_RESID_F32>(c, w->attn.as<op_t>(), d, 0, Wb + ly.out_w, (int)M, d, d, Wf + ly.out_b, w->resid.as<float>(), d, 0, 1);
        {
            KernelTimer kt(c, PCE_K_LAYERNORM);
            launch_layernorm<op_t>(c, w->resid.as<float>(), Wf + ly.ln2_w, Wf + ly.ln2_b, M, d, w->ln_out.as<op_t>());
        }
        launch_gemm<EPI_GELU_BF16>(c, w->ln_out.as<op_t>(), d, 0, Wb + ly.m1_w, (int)M, 4 * d, d, Wf + ly.m1_b, w->hidden.as<op_t>(), 4 * d, 0, 1);
        launch_gemm<EPI_RESID_F32>(c, w->hidden.as<op_t>(), 4 * d, 0, Wb + ly.m2_w, (int)M, d, 4 * d, Wf + ly.m2_b, w->resid.as<float>(), d, 0, 1);
    }
    if (!flat) {
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
    PCE_HIP(c, hipMemcpyAsync(out, w->final_out.as<float>() + per * (size_t)clip, sizeof(float) * per, hipMemcpyDeviceToHost, c->stream));
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

} // extern "C"

#include "pce_whisper_decoder.inc"
#include "pce_whisper_selftest.inc"      // (after the decoder: pce_selftest_decode_rules shares its launch helpers)
#include "pce_bert.inc"
#include "pce_w2v.inc"
