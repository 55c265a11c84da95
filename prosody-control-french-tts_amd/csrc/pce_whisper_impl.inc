// pce_whisper_impl.inc -- the transformer work of the alignment step (R8) on gfx950: log-mel spectrogram, Whisper audio encoder,
// text decoder (teacher-forced forced alignment with cross-attention DTW; free-running greedy decoding with a K / V
// cache and openai-whisper's logit filters), and the break-prediction BERT forward, which shares the same kernels.
// This file: the types and constants every part shares; the kernels, included by theme in the order the unit defines them (pce_logmel.inc,
// pce_gemm_tiled.inc, pce_layernorm.inc, pce_gemm256.inc, pce_attention.inc, pce_decode_kernels.inc, pce_xattn.inc, pce_decode_rules.inc,
// pce_align_kernels.inc); WhisperState, the device half of the weight loaders (upload_weights; pce_weight_pack.h is the host half), the launchers that sit
// behind several of those files, the log-mel entry points; it ends by including the other entry points: pce_encoder.inc (the encoder layer walk, the Whisper
// encoder), pce_whisper_decoder.inc, pce_whisper_selftest.inc, pce_bert.inc, pce_w2v.inc (one translation unit per operand type).
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
#include "pce_weight_pack.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <optional>
#include <type_traits>

// This file is compiled twice (pce_whisper_bf16.hip, pce_whisper_f16.hip): PCE_OP_T is the 16-bit operand type of every GEMM / attention
// product (fp32 accumulation and an fp32 residual stream in both builds), PCE_OP_INDEX the slot of the context that holds this build's
// state, PCE_BUILD_NS the namespace (pce_bf16 / pce_f16) the build defines its entry points in, with C++ linkage; pce_whisper_dispatch.hip
// exports the names of include/pce.h and forwards to the build the context selects (pce_whisper_set_operands).  The entry points are listed
// once, in pce_whisper_entries.h.  Every kernel stays in the anonymous namespace at file scope (its name is part of the code object); host-only
// helpers may sit in either.
// bf16: the round-1 / round-2 arithmetic.  fp16: the reference's own -- openai-whisper runs the model in half precision (fp16 activations and
// weights, fp32 LayerNorm and softmax; transcribe's fp16=True default behind Code/Aligners/use_whisper_timestamped.py:163): 11 significand bits
// instead of 8 at the same MFMA rate.
#include "pce_whisper_entries.h"
namespace PCE_BUILD_NS {
PCE_WHISPER_ENTRIES(PCE_DECLARE)
}

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

#include "pce_logmel.inc"
#include "pce_gemm_tiled.inc"
#include "pce_layernorm.inc"
#include "pce_gemm256.inc"

#include "pce_attention.inc"
#include "pce_decode_kernels.inc"
#include "pce_xattn.inc"

#include "pce_decode_rules.inc"
#include "pce_align_kernels.inc"

__global__ void k_f32_to_bf16(const float *__restrict__ in, op_t *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (op_t)in[i];
}
// The device half of a loader: pk.mats through `tmp` into w16 as op_t, pk.vecs into w32.  Everything is enqueued on the context's stream: the caller
// synchronises it before `tmp` goes out of scope.
static int upload_weights(pce_ctx *c, const WeightPack &pk, DevBuf &tmp, DevBuf &w16, DevBuf &w32)
{
    PCE_UPLOAD(c, tmp, pk.mats);
    PCE_UPLOAD(c, w32, pk.vecs);
    PCE_HIP(c, w16.reserve(sizeof(op_t) * pk.mats.size() + 256));
    hipLaunchKernelGGL(k_f32_to_bf16, dim3((unsigned)div_up((int64_t)pk.mats.size(), 256)), dim3(256), 0, c->stream, tmp.as<float>(), w16.as<op_t>(),
                       (int64_t)pk.mats.size());
    return PCE_OK;
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

// one transformer encoder layer's offsets (elements) into the operand-type and fp32 weight buffers of its model: Whisper's audio encoder, BERT, wav2vec2
struct EncoderLayerW { size_t ln1_w, ln1_b, qkv_w, qkv_b, out_w, out_b, ln2_w, ln2_b, m1_w, m1_b, m2_w, m2_b; };

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
        std::vector<EncoderLayerW> layers;
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
        std::vector<EncoderLayerW> layers;
        size_t fp_ln_w = 0, fp_ln_b = 0, proj_w = 0, proj_b = 0, pos_w = 0, pos_b = 0, enc_ln_w = 0, enc_ln_b = 0, lm_w = 0, lm_b = 0;
        int Vp = 0;                         // lm_head's columns, padded to whole GEMM tiles
        DevBuf img[2], part, ss, wintab, tailtab, atab, t0tab, fpln, h0, h, ln, qk, vt, attn, hidden, logits, em;
        std::vector<int64_t> row_start;     // first row of clip q in em
        std::vector<int32_t> n_frames;
        int n_cols = 0, n_clips = -1;       // n_clips < 0: no run yet
        int64_t seg_plan[3] = {-1, 0, 0};   // the latest pce_w2v_run_segments: chunks, rows computed, rows valid (chunks < 0: the latest run was none)
    } w2v;
    // offsets (elements) into w_bf16 / w_f32
    size_t c1_w = 0, c1_b = 0, c2_w = 0, c2_b = 0, lnp_w = 0, lnp_b = 0;
    std::vector<EncoderLayerW> layers;
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
    int rc = PCE_OK;
    auto put = [&](const auto &v) -> const void * {                // every table starts at a multiple of 16 bytes; the first failed copy is kept
        if (!rc) rc = pce_put_at(c, __FILE__, __LINE__, d + o, v.data(), v.size());
        const void *p = d + o; o += (sizeof(v[0]) * v.size() + 15) & ~(size_t)15; return p;
    };
    w->mt.w16 = (const float2 *)put(w16);
    w->mt.w400 = (const float2 *)put(w400);
    w->mt.w25 = (const float2 *)put(w25);
    w->mt.window = (const float *)put(win);
    w->mt.mel_lo = (const int *)put(lo);
    w->mt.mel_n = (const int *)put(cnt);
    w->mt.mel_off = (const int *)put(off);
    w->mt.mel_w = (const float *)put(packed);
    w->mt.mel_total = (int)packed.size();
    PCE_TRY(rc);
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
    if (!c->sw.gemm_flat || N % F_T || K % F_K || M < 1 || N > F_N_MAX || (HAS_VT && (S % 4 || S < F_T))) return false;
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
    if (c->sw.gemm_skinny && c->gemm_few_rows && gemm_fits<EPI>(GK_SKINNY, s)) return GK_SKINNY;
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

namespace PCE_BUILD_NS {

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
    PCE_TRY(mel_setup(c, w, n_mels));
    const int32_t n = c->n_clips;
    const size_t tm_elems = (size_t)n * (W_FRAMES + 2) * (size_t)n_mels + 512;
    PCE_HIP(c, w->logspec.reserve(sizeof(float) * (size_t)n * (size_t)n_mels * W_FRAMES));
    PCE_HIP(c, w->mel_tm.reserve(sizeof(op_t) * tm_elems));
    PCE_HIP(c, w->stem_skip.reserve(sizeof(int2) * 2 * (size_t)(n > 0 ? n : 1)));
    w->stem_tiles_c1 = w->stem_tiles_c2 = 0;
    for (int32_t i = 0; i < n; i++) {      // what k_logmel_norm will write per clip, summed from the host's copy of the same lengths and starts
        const int64_t full = c->clip_off[(size_t)i + 1] - c->clip_off[(size_t)i];
        const int s = stem_first_skipped_tile(start_frames ? full : std::min<int64_t>(full, W_SAMPLES), start_frames ? start_frames[i] : 0);
        if (s < ST_C2_LAST) { w->stem_tiles_c2 += ST_C2_LAST - s; w->stem_tiles_c1 += ST_C1_KEEP - 2 * s; }
    }
    PCE_ZERO(unsigned int, c, w->clipmax, (size_t)n);
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
        PCE_UPLOAD(c, w->mel_start, start_frames, (size_t)n, n > 0 ? 0 : 1);
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
    PCE_FETCH(c, out, w->mel_stage.p, per);
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
    PCE_FETCH(c, out, w->mel_tm.as<op_t>() + (size_t)clip * per, per);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    return PCE_OK;
}

} // namespace PCE_BUILD_NS

#include "pce_encoder.inc"
#include "pce_whisper_decoder.inc"
#include "pce_whisper_selftest.inc"      // (after the decoder: pce_selftest_decode_rules shares its launch helpers)
#include "pce_bert.inc"
#include "pce_w2v.inc"
