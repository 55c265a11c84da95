// pce_internal.h -- shared between the translation units of libpce.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "pce.h"
#include "pce_sweep_plan.h"
#include "pce_pitch_plan.h"

// A kernel marked PCE_NO_PK_F32 is compiled without packed fp32 instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32).  Why (round 6,
// profiles/r06/multiprocess_glitch.txt, tools/lab/pk_victim.hip): on the MI355X boxes of this pool a packed fp32 instruction whose low result lane
// reads src0's LOW half and src1's HIGH half (op_sel:[0,1]) returns wrong values in lanes 48..63 while another wave on the same SIMD executes MFMA.
// The compiler forms exactly that selection for complex products and for pair sums; tools/isa_guard.py refuses a library that holds one.
#if defined(__HIP_DEVICE_COMPILE__)
#define PCE_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define PCE_NO_PK_F32                                    /* (the host pass of the same source: an x86 target knows no such feature) */
#endif

// Growable device buffer; frees itself.  Never give one static storage duration: its destructor would call hipFree after the runtime has shut down.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf &operator=(DevBuf &&o) noexcept {         // frees what this one held, takes o's allocation
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + (bytes >> 3) + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Last slice list an op was planned for: a repeated *_run with the same slices
// (the steady state of a batch pipeline, and of bench.py) skips the host plan.
struct SliceCache {
    std::vector<pce_slice> v;
    bool valid = false;
    bool same(const pce_slice *s, int32_t n) const {
        return valid && (size_t)n == v.size() && (n == 0 || memcmp(v.data(), s, sizeof(pce_slice) * (size_t)n) == 0);
    }
    void store(const pce_slice *s, int32_t n) { v.assign(s, s + n); valid = true; }
    void drop() { valid = false; v.clear(); }
};

struct pce_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // side streams: work that leaves most of the machine idle (or is independent of what the caller launches next) is
    // forked from `stream` onto one of these and joined back by whoever consumes its results:
    //   SIDE_TAIL  path finder + median of the pitch analysis (latency bound, ~0.4 ms with few CUs busy)
    //   SIDE_LUFS  the LUFS chain (sequential IIR per lane: few waves, long dependent chains)
    //   SIDE_STFT  the HBM-bound normalisation pass of the STFT-dB (the FFT pass itself stays on `stream`: launched
    //              beside the pitch kernels it only competed for VALU issue, 3.33 -> 3.54 ms)
    enum { SIDE_TAIL = 0, SIDE_LUFS = 1, SIDE_STFT = 2, SIDE_COUNT = 3 };
    struct Side { hipStream_t s = nullptr; hipEvent_t fork = nullptr, join = nullptr; bool pending = false; } side[SIDE_COUNT];
    // what pce_create reads from the environment, once (switches_from_env, pce_ctx.hip)
    struct Switches {
        bool no_side = false;                // PCE_NO_AUX at pce_create: everything on `stream`
        bool generic_median = false;         // PCE_ALIGN_GENERIC_MEDIAN at pce_create: the insertion-sort median filter for every width
        bool gemm_skinny = true;             // PCE_GEMM_SKINNY=0 at pce_create: few-row launches stay on the 128 x 128 kernel
        bool gemm_flat = true;               // PCE_GEMM_FLAT=0 at pce_create: the encoder's projections stay on the 128 x 128 / 128 x 256 tile kernels
        int resid_epilogue = 1;              // PCE_RESID_EPILOGUE at pce_create: 0 = the 16-bit-stream encoder stores its branch outputs and adds them in k_add_layernorm (A/B, bit-identity
                                             // test), 2 = only fc2 adds in its epilogue (the per-shape A/B of DESIGN.md section 4); default 1: the attention projection and fc2 do
        bool stem_skip = true;               // PCE_STEM_SKIP=0 at pce_create: the conv stem multiplies every row of the 30 s window, the zero padding's included (A/B, bit-identity test)
        bool stft_two_fft = false;           // PCE_STFT_TWO_FFT at pce_create: traffic-minimal STFT-dB (the FFT runs twice)
        int en_cpb = 0;                      // PCE_EN_CPB: chunks per k_energy workgroup (0 = by batch size)
        bool xattn_absorb = true;            // incremental decoding steps: cross-attention from the encoder output (pce_xattn.inc); PCE_XATTN_ABSORB=0: from the K / V^T cache
        bool self_rows = true;               // incremental steps' self-attention on row-major K / V caches (k_self_attn1w); PCE_SELF_ROWS=0: k_cross_attn1w on K rows + V^T
        size_t dtw_trace_budget = (size_t)4096 << 20;   // PCE_DTW_TRACE_MB at pce_create: bytes of trace one group of pairs may hold
        size_t ctc_trace_budget = (size_t)4096 << 20;   // PCE_CTC_TRACE_MB at pce_create: bytes of trace one group of clips may hold
        size_t ivl_table_budget = (size_t)2048 << 20;   // PCE_IVL_TABLE_MB at pce_create: bytes of class tables one group of table pairs may hold
    } sw;
    bool pitch_refine_praat = false;     // PCE_PITCH_REFINE=praat at pce_create: the candidate refinement replays NUMminimize_brent's own iterates (round 1 / 2 behaviour)
    bool gemm_few_rows = false;          // set by the incremental decoding step around its launches: k_gemm_skinny is eligible
    std::string err;
    int cu_count = 0;

    // resident batch
    DevBuf pcm_own;                 // used by pce_upload_pcm_s16
    const int16_t *d_pcm = nullptr; // device pointer to the concatenated clips
    DevBuf d_clip_off;              // int64[n_clips+1]
    std::vector<int64_t> clip_off;  // host copy
    int32_t n_clips = 0;
    int32_t rate = 0;

    // energy
    DevBuf en_work, en_out;
    SliceCache en_cache;
    int64_t en_n_work = 0;
    int32_t en_n = -1;

    // lufs
    DevBuf lu_meta, lu_chunks, lu_blocks, lu_pow, lu_state_end, lu_state_init, lu_energy, lu_zbuf, lu_out, lu_en_work, lu_en_acc;
    SliceCache lu_cache;
    int64_t lu_n_chunks = 0, lu_n_blocks = 0, lu_n_energy_work = 0;
    double lu_coef[13] = {0};
    int32_t lu_n = -1;
    int32_t lu_meter_rate = 0;       // pce_lufs_set_meter_rate: 0 = the batch's own rate
    bool lu_reads_en_out = false;    // the running LUFS chain takes its peaks from pce_energy_run's accumulators (same slices)
    bool lu_peaks_in_en_out = false; // the latest pce_lufs_run took them from there (pce_lufs_fetch_stages; lu_reads_en_out is cleared by the next energy run)
    std::vector<int32_t> lu_host_status;

    // pitch
    DevBuf pi_meta, pi_window, pi_windowR, pi_work, pi_cand, pi_gpeak, pi_psi, pi_f0, pi_strength, pi_summary, pi_peakwork, pi_acc, pi_rr, pi_items, pi_tw, pi_dl, pi_runs, pi_fslice, pi_blob;
    PiParams pi_P = {};                 // what the kernels take by value (pce_pitch_plan.h)
    PitchFramesLaunch pi_launch = {};   // the k_pitch_frames launch planned with it
    PitchSizes pi_sizes = {};           // ... and the list capacities and buffer sizes
    int64_t pi_n_work = 0, pi_n_energy_work = 0;
    int pi_np2 = 1;
    bool pi_long_slices = false;    // some slice has more frames than the in-LDS median sort holds (k_pitch_median_long takes those)
    SliceCache pi_cache;
    pce_pitch_params pi_params;
    bool pi_params_valid = false;
    int32_t pi_n = -1;
    int64_t pi_total_frames = 0;
    std::vector<int64_t> pi_frame_off;
    std::vector<int32_t> pi_status;
    std::vector<double> pi_t1;

    // stft
    DevBuf st_out, st_max, st_off, st_window, st_twiddle, st_work, st_stage;   // st_stage: one clip's finished values on their way to the host (pce_stft_db_fetch)
    int32_t st_nfft = 0, st_hop = 0;
    int64_t st_n_tiles = 0;
    bool st_ran = false;
    bool st_final = false;            // st_out holds finished values (ref = max applied): after the two-FFT form or pce_stft_db_device; raw dB + st_max otherwise
    std::vector<int64_t> st_off_host;   // float offsets per clip (n_clips+1)
    std::vector<int32_t> st_frames;

    // frame energy (analysis windows of the energy VAD)
    DevBuf fr_doff, fr_sum, fr_cnt;
    std::vector<int64_t> fr_off;        // frames before clip i (n_clips+1)
    bool fr_ran = false;

    // probabilistic YIN
    DevBuf py_doff, py_tab, py_hdr, py_bin, py_lp, py_ptr, py_states;
    std::vector<int64_t> py_off;
    bool py_ran = false;

    // CREPE pitch tracking (pce_crepe.hip): folded weights, the padded time-major operand images of one chunk of frames, salience and decoding of the whole batch
    struct Crepe {
        bool loaded = false, ran = false;
        int c_out[6] = {0}, c_in[6] = {0}, n_emb = 0;
        int decoder = 0;
        DevBuf w16[6], bss[6], cls_w, cls_b;            // conv weights [out][taps][in] fp16; bias | scale | shift fp32 [3][out]; classifier fp32
        DevBuf img[7];                                  // img[0]: block 1's frames; img[i]: block i + 1's padded input; img[6]: the embedding
        DevBuf doff, P, logp, ptr, amax, bins, f0, per, tab;
        std::vector<int64_t> off;                       // frames before clip i (n_clips + 1)
    } cr;

    // Praat intensity (pce_intensity.hip): slice table, runs of frames, the tap table, the ragged contour, per-slice {n_positive, mean_positive}
    DevBuf in_meta, in_work, in_taps, in_out, in_summary;
    SliceCache in_cache;
    pce_intensity_params in_params;
    bool in_params_valid = false;
    std::vector<double> in_taps_host;    // the table the plan was made for
    int in_hs = 0, in_fpb = 0, in_span = 0;
    double in_dt = 0.0;
    size_t in_lds = 0;
    int64_t in_n_work = 0, in_total_frames = 0;
    int32_t in_n = -1;
    std::vector<int64_t> in_frame_off;
    std::vector<int32_t> in_status;
    std::vector<double> in_t1;

    // silence detection (pce_silence.hip): slice table, in-chunk prefix sums of the millisecond bins, chunk totals and offsets, tile summaries and
    // carries of the range pass, the ranges at their per-slice bound, the per-slice range counts
    DevBuf si_meta, si_pl, si_csum, si_coff, si_tsum, si_tin, si_out, si_count;
    std::vector<int32_t> si_len_ms, si_status, si_counts;
    std::vector<int64_t> si_cap_off;     // ranges the slices before slice i may have (n + 1)
    bool si_counts_valid = false;
    int32_t si_n = -1;

    // DTW of series pairs (pce_dtw_series.hip): the batch's inputs and results, the tables of the group in flight, its boundary rows / columns and trace
    struct DtwSeries { DevBuf a, b, lo, hi, pi, pj, dist, len, status, pairs, tab, tiles, rows, cols, trace; } ds;

    // CTC forced alignment (pce_ctc.hip): uploaded emissions, clip table, clip-id lists, targets, final alphas, the trace of the group in flight, the general
    // form's alpha rows, the batch's results
    struct Ctc { DevBuf lp, tab, ids, tgt, fin, trace, scratch, path, fscore, first, last, score, status; } ctc;

    // whisperX alignment (pce_wx.hip): uploaded emissions, clip table, clip-id lists, tokens, the wildcard's row maxima, the trellis tables of the group in
    // flight, the back-track's record (8 words per frame), the batch's results
    struct Wx { DevBuf lp, tab, ids, tok, wmax, table, rec, path, plp, score, status; } wx;

    // whisper / BERT state, opaque (pce_whisper_impl.inc): one slot per operand-type build (0: bf16, 1: fp16); whisper_ops selects the build the
    // entry points of include/pce.h forward to (pce_whisper_set_operands, or PCE_WHISPER_OPERANDS=fp16 at pce_create)
    void *whisper_slot[2] = {nullptr, nullptr};
    int whisper_ops = 2;                 // (pce_create: 2 = the fp16 build + resid16 unless PCE_WHISPER_OPERANDS=bf16 / fp16)
    bool resid16 = true;                 // the batched encoder path keeps its residual stream in 16 bits (fp16 build only)

    // asynchronous statistics fetch (pce_stats_enqueue / pce_stats_wait)
    struct StatSlot {
        void *host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr, ev_main = nullptr; bool armed = false;
        int32_t en_n = -1, lu_n = -1, pi_n = -1;
        size_t off_lu = 0, off_pi = 0;
        std::vector<int64_t> en_len, pi_frames;
        std::vector<int32_t> lu_status, pi_status;
        std::vector<double> pi_t1;
    } stat[2];

    // profiling
    bool prof = false;
    double prof_ms[PCE_K_COUNT] = {0};
    int64_t prof_n[PCE_K_COUNT] = {0};
    double prof_flops[PCE_K_COUNT] = {0};
    struct Pending { int id; hipEvent_t a, b; double flops; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
};

int pce_fail(pce_ctx *ctx, int code, const char *fmt, ...);
#define PCE_HIP(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return pce_fail((ctx), PCE_E_DEVICE, "%s: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)
#define PCE_TRY(expr) do { const int rc__ = (expr); if (rc__) return rc__; } while (0)

// Host <-> device staging on c->stream.  Counts are in ELEMENTS of T, the only multiplications by sizeof(T) are the ones below, and a failure reads like
// PCE_HIP's, with the caller's file and line.  A helper takes a buffer's .p only after its own reserve; none synchronises.
int pce_stage_fail(pce_ctx *c, const char *what, hipError_t e, const char *file, int line);
int pce_stage_copy(pce_ctx *c, void *dst, const void *src, size_t bytes, hipMemcpyKind kind, const char *file, int line);
// reserve count + slack elements in b, copy count of them from the host (src == nullptr with count == 0: reserve only)
template <class T> static inline int pce_upload_at(pce_ctx *c, const char *file, int line, DevBuf &b, const T *src, size_t count, size_t slack = 0)
{
    const hipError_t e = b.reserve(sizeof(T) * (count + slack));
    if (e != hipSuccess) return pce_stage_fail(c, "reserve", e, file, line);
    return count ? pce_stage_copy(c, b.p, src, sizeof(T) * count, hipMemcpyHostToDevice, file, line) : PCE_OK;
}
template <class T> static inline int pce_upload_at(pce_ctx *c, const char *file, int line, DevBuf &b, const std::vector<T> &src, size_t slack = 0)
{
    return pce_upload_at(c, file, line, b, src.data(), src.size(), slack);
}
// count elements from the host into a range of a buffer that is already reserved
template <class T> static inline int pce_put_at(pce_ctx *c, const char *file, int line, void *dst, const T *src, size_t count)
{
    return pce_stage_copy(c, dst, src, sizeof(T) * count, hipMemcpyHostToDevice, file, line);
}
// reserve count + slack elements of T in b, zero the first count
template <class T> static inline int pce_zero_at(pce_ctx *c, const char *file, int line, DevBuf &b, size_t count, size_t slack = 0)
{
    hipError_t e = b.reserve(sizeof(T) * (count + slack));
    if (e == hipSuccess && count) e = hipMemsetAsync(b.p, 0, sizeof(T) * count, c->stream);
    return e == hipSuccess ? PCE_OK : pce_stage_fail(c, "reserve + memset", e, file, line);
}
// count elements back to the host
template <class T> static inline int pce_fetch_at(pce_ctx *c, const char *file, int line, T *dst, const void *src, size_t count)
{
    return pce_stage_copy(c, dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, file, line);
}
#define PCE_UPLOAD(c, ...) PCE_TRY(pce_upload_at((c), __FILE__, __LINE__, __VA_ARGS__))
#define PCE_PUT(c, ...) PCE_TRY(pce_put_at((c), __FILE__, __LINE__, __VA_ARGS__))
#define PCE_ZERO(T, c, ...) PCE_TRY(pce_zero_at<T>((c), __FILE__, __LINE__, __VA_ARGS__))
#define PCE_FETCH(c, ...) PCE_TRY(pce_fetch_at((c), __FILE__, __LINE__, __VA_ARGS__))

// What pce_ctc_align and pce_wx_align do alike before their launches (pce_ctx.hip).  `fn` is the entry point's name and `seq` what it calls its label
// sequences ("target" / "token"), for the messages.
struct SweepScan { int64_t row_lo = INT64_MAX, row_hi = 0, total_frames = 0; };     // emission rows [row_lo, row_hi) are read; frames of all clips
int pce_sweep_check(pce_ctx *c, const char *fn, const int64_t *row_start, const int32_t *n_frames, const int64_t *seq_off, const void *p, const float *score,
                    const int32_t *status, int32_t n_clips, int32_t n_vocab, int32_t blank);
// clip q into cl: rows, offsets, frames and length (stride, st0, scr0, wild: the caller's), and into the batch's totals
int pce_sweep_scan_clip(pce_ctx *c, const char *fn, const char *seq, size_t q, const int64_t *row_start, const int32_t *n_frames, const int64_t *seq_off, SweepScan &s,
                        SweepClip &cl);
// host emissions: rows [row_lo, row_hi) go to buf and the table's rows shift; -> the device pointer the kernels read
int pce_sweep_stage_emissions(pce_ctx *c, DevBuf &buf, const float *emissions, int32_t on_device, int32_t n_vocab, const SweepScan &s, std::vector<SweepClip> &tab,
                              const float **d_lp);

// Kernel-launch bracket for the profiler: records events around the launch when enabled.
struct KernelTimer {
    pce_ctx *c; int id; hipEvent_t a = nullptr, b = nullptr; hipStream_t s; double flops;
    KernelTimer(pce_ctx *ctx, int kid, hipStream_t on = nullptr, double work_flops = 0.0);
    ~KernelTimer();
};
void pce_profile_collect(pce_ctx *ctx, bool wait = true);
int pce_join_aux(pce_ctx *c);                                // make `stream` wait for ALL pending side-stream work
int pce_side_join(pce_ctx *c, int which);                    // ... for one side stream
int pce_side_begin(pce_ctx *c, int which, hipStream_t *out); // fork: *out = side stream ordered behind `stream` (or `stream` itself: PCE_NO_AUX)
int pce_side_end(pce_ctx *c, int which, hipStream_t used);   // record the join point   // wait = false: only the launches that have completed

// staged fetch helpers of the modules (pce_stats_*): bytes needed, enqueue the copy into pinned memory, unpack it
size_t pce_energy_stage_bytes(const pce_ctx *c);
int pce_energy_stage_enqueue(pce_ctx *c, void *pinned, std::vector<int64_t> &lens);
void pce_energy_stage_unpack(const void *pinned, const std::vector<int64_t> &lens, pce_energy *out);
size_t pce_pitch_stage_bytes(const pce_ctx *c);
int pce_pitch_stage_enqueue(pce_ctx *c, void *pinned, hipStream_t on = nullptr);
void pce_pitch_stage_unpack(const void *pinned, int32_t n, pce_pitch_summary *out);

// the integer pass over slices (pce_energy.hip) as the pitch and LUFS paths run it into buffers of their own: plan the work list, launch, and where
// a slice's sum / extrema lie in out_buf
int pce_energy_plan(pce_ctx *c, const pce_slice *slices, int32_t n, DevBuf &work_buf, DevBuf &out_buf, int64_t *n_work);
int pce_energy_launch(pce_ctx *c, int32_t n, int32_t loud_thr, int64_t n_work, DevBuf &work_buf, DevBuf &out_buf, hipStream_t on = nullptr);
void pce_energy_range_ptrs(const DevBuf &out_buf, size_t *stride_bytes, const long long **sum, const int **m_hi, const int **m_lo);

void pce_whisper_free(pce_ctx *c);
static inline int64_t div_up(int64_t a, int64_t b) { return (a + b - 1) / b; }
