// pce_intensity.hip -- k_intensity / k_intensity_summary: Praat's Sound_to_Intensity over slices of the resident batch.
//
// Reference call replaced: parselmouth Sound.to_intensity() of Code/visualisation/Compare_speech_noenhanced.py:19-26 (extract_mean_volume)
// and of the 'volume' branch of its plot_zscore_feature / plot_raw_feature (:166-168, :300-302).  parselmouth and the Praat sources are
// absent: this is a restatement of the published algorithm (Sound_to_Intensity.cpp), parity with Praat unpinned.
//
//   window = 6.4 / pitch_floor, half = window / 2, hs = floor(half / dx), 2 hs + 1 taps w[k] = I0f((2 pi^2 + 0.5) sqrt(1 - (k dx / half)^2))
//   (the table is host logic: hostrules.intensity_window; the kernel and a checker read the same doubles);
//   frames by Sampled_shortTermAnalysis (window, time step); frame f: centre = the sample nearest t1 + f dt, span = centre +- hs CLIPPED
//   to the slice (Praat clips: the weight sum shrinks with the clip; this is not the virtual-zero rule of the other analyses -- samples of
//   the slice that lie outside its clip are still zeros); mean = unweighted mean of the span (exact integer numerator);
//   I = sum (a - mean)^2 w / sum w / 4e-10; value = I < 1e-30 ? -300 : 10 log10 I.  Everything in fp64.
//
// Shape: a workgroup owns a run of up to IN_FPB consecutive frames of one slice.  It stages the tap table (<= 48 KB) and the int16 samples
// under its frames (16-byte loads, <= 64 KB) in LDS once; frames overlap 8 x at the default time step, so a sample leaves HBM / L2
// 1 + (taps - 1) / (IN_FPB hop) times (1.25 at the defaults) instead of 8.  Each wave then takes whole frames: lane l accumulates taps
// l, l + 64, ... in order, the 64 partial sums meet in a fixed xor butterfly.  No atomics: a frame's bits depend on its own samples only.
// Bound: LDS reads (10 bytes per tap and frame) and the dependent fp64 adds, not HBM.
#include "pce_internal.h"
#include "pce_wave.h"
#include <cmath>

namespace {

constexpr int IN_THREADS = 256;
constexpr int IN_FPB = 32;                // frames per workgroup (fewer when their samples would not fit IN_MAX_SPAN)
constexpr int IN_MAX_TAPS = 6145;         // pitch_floor 50 Hz at 48 kHz
constexpr int IN_MAX_SPAN = 32768;        // int16 samples staged per workgroup

struct InSlice { int64_t begin, clip_len, clip_off, nx, frame_off; double x1, t1; int32_t n_frames, status; };
struct InWork { int32_t slice, frame0; };
struct InParams { double dx, dt; int hs, fpb, span, subtract_mean; };
struct InSummaryDev { long long n_positive; double mean_positive; };

// Sampled_indexToX of the Intensity, then Sampled_xToNearestIndex of the Sound (Melder_iround = floor(x + 0.5)), 0-based
__device__ __forceinline__ int64_t in_centre(const InSlice &s, const InParams &P, int frame)
{
    const double t = s.t1 + (double)frame * P.dt;
    return (int64_t)floor(((t - s.x1) / P.dx + 1.0) + 0.5) - 1;
}

__global__ __launch_bounds__(IN_THREADS) void k_intensity(const int16_t *__restrict__ pcm, const InSlice *__restrict__ slices,
                                                         const InWork *__restrict__ work, const double *__restrict__ taps, InParams P,
                                                         double *__restrict__ out)
{
    typedef int i4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) double in_lds[];
    const int n_taps = 2 * P.hs + 1;
    double *w = in_lds;                                                        // [n_taps], padded to an even count
    int16_t *sp = reinterpret_cast<int16_t *>(in_lds + ((n_taps + 1) & ~1));   // [P.span + 8], 16-byte aligned
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const InWork wk = work[blockIdx.x];
    const InSlice s = slices[wk.slice];
    const int nfr = min(P.fpb, s.n_frames - wk.frame0);

    for (int i = threadIdx.x; i < n_taps; i += IN_THREADS) w[i] = taps[i];

    // samples under this run of frames, slice coordinates [lo, hi]
    const int64_t lo = max(in_centre(s, P, wk.frame0) - P.hs, (int64_t)0);
    const int64_t hi = min(in_centre(s, P, wk.frame0 + nfr - 1) + P.hs, s.nx - 1);
    const int n_stage = (int)min(hi - lo + 1, (int64_t)P.span);
    // 16-byte groups of the concatenated PCM; sample `lo` sits at sp[sh].  A group is loaded when any of it lies in the clip and
    // masked per sample: what the slice holds outside its clip is zero.
    const int64_t gs = s.clip_off + s.begin + lo;
    const int64_t a0 = gs & ~(int64_t)7;
    const int sh = (int)(gs - a0);
    const int64_t c_lo = s.clip_off, c_hi = s.clip_off + s.clip_len;
    const int n_groups = n_stage > 0 ? (sh + n_stage + 7) >> 3 : 0;
    for (int g = threadIdx.x; g < n_groups; g += IN_THREADS) {
        const int64_t p = a0 + 8 * (int64_t)g;
        i4 v = (i4){0, 0, 0, 0};
        if (p + 8 > c_lo && p < c_hi) {
            v = *reinterpret_cast<const i4 *>(pcm + p);
            if (p < c_lo || p + 8 > c_hi) {
                int words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int64_t j0 = p + 2 * q, j1 = j0 + 1;
                    const unsigned keep = ((j0 >= c_lo && j0 < c_hi) ? 0x0000FFFFu : 0u) | ((j1 >= c_lo && j1 < c_hi) ? 0xFFFF0000u : 0u);
                    words[q] &= (int)keep;
                }
                v = (i4){words[0], words[1], words[2], words[3]};
            }
        }
        *reinterpret_cast<i4 *>(sp + 8 * g) = v;
    }
    __syncthreads();

    for (int fi = wv; fi < nfr; fi += IN_THREADS / 64) {
        const int frame = wk.frame0 + fi;
        const int64_t c = in_centre(s, P, frame);
        const int64_t l = max(c - P.hs, (int64_t)0), r = min(c + P.hs, s.nx - 1);
        const int n = (int)(r - l + 1);
        double value = -300.0;
        // (l - lo >= 0 and r <= hi: centres do not decrease with the frame; n_stage bounds what was staged)
        if (n > 0 && l >= lo && r - lo < n_stage) {
            const int16_t *x = sp + sh + (int)(l - lo);
            const double *wt = w + (int)(l - c + P.hs);
            double mean = 0.0;
            if (P.subtract_mean) {
                int isum = 0;                                  // |sum| <= 6145 x 32768 < 2^31
                for (int k = lane; k < n; k += 64) isum += (int)x[k];
                isum = wave_xor_sum(isum);
                mean = ((double)isum / 32768.0) / (double)n;
            }
            double num = 0.0, den = 0.0;
            for (int k = lane; k < n; k += 64) {
                const double d = (double)x[k] / 32768.0 - mean;
                const double wk_ = wt[k];
                num += (d * d) * wk_;
                den += wk_;
            }
            num = wave_xor_sum(num); den = wave_xor_sum(den);
            const double I = num / den / 4.0e-10;
            value = I < 1.0e-30 ? -300.0 : 10.0 * log10(I);
        }
        if (lane == 0) out[s.frame_off + frame] = value;
    }
}

// {n_positive, mean of the values > 0 (NaN when none)} per slice: one wave per slice, lane l adds frames l, l + 64, ... in order, then
// the same butterfly.  What extract_mean_volume computes (values[values > 0], np.nanmean).
__global__ __launch_bounds__(64) void k_intensity_summary(const InSlice *__restrict__ slices, const double *__restrict__ values,
                                                         InSummaryDev *__restrict__ out)
{
    const InSlice s = slices[blockIdx.x];
    const int lane = threadIdx.x;
    int np = 0; double sum = 0.0;
    for (int f = lane; f < s.n_frames; f += 64) {
        const double v = values[s.frame_off + f];
        if (v > 0.0) { np++; sum += v; }
    }
    np = wave_xor_sum(np); sum = wave_xor_sum(sum);
    if (lane == 0) {
        out[blockIdx.x].n_positive = np;
        out[blockIdx.x].mean_positive = np > 0 ? sum / (double)np : __builtin_nan("");
    }
}

struct InPlan { double window, dt, t1; int64_t n_frames; };

// Sampled_shortTermAnalysis with the window and time step of Sound_to_Intensity
int intensity_plan_make(int64_t nx, double dx, double x1, const pce_intensity_params *p, InPlan *pl)
{
    pl->window = 6.4 / p->pitch_floor;
    pl->dt = p->time_step <= 0.0 ? 0.8 / p->pitch_floor : p->time_step;
    const double myDuration = dx * (double)nx;
    if (pl->window > myDuration) return PCE_SLICE_TOO_SHORT;
    pl->n_frames = (int64_t)std::floor((myDuration - pl->window) / pl->dt) + 1;
    if (pl->n_frames < 1) return PCE_SLICE_TOO_SHORT;
    const double ourMidTime = x1 - 0.5 * dx + 0.5 * myDuration;
    const double thyDuration = (double)pl->n_frames * pl->dt;
    pl->t1 = ourMidTime - 0.5 * thyDuration + 0.5 * pl->dt;
    return PCE_SLICE_OK;
}

int intensity_plan_slices(pce_ctx *c, const pce_intensity_params *p, const pce_slice *slices, int32_t n, std::vector<int64_t> &frame_off,
                          std::vector<int32_t> &status, std::vector<double> &t1)
{
    if (!(p->pitch_floor > 0.0) || !std::isfinite(p->pitch_floor) || !std::isfinite(p->time_step))
        return pce_fail(c, PCE_E_INVALID, "intensity: pitch_floor must be positive and finite, time_step finite");
    const double dx = 1.0 / (double)c->rate;
    frame_off.assign((size_t)n + 1, 0); status.assign((size_t)n, PCE_SLICE_OK); t1.assign((size_t)n, 0.0);
    for (int32_t i = 0; i < n; i++) {
        const pce_slice &s = slices[i];
        if (s.clip < 0 || s.clip >= c->n_clips) return pce_fail(c, PCE_E_INVALID, "slice %d: clip %d out of range", i, s.clip);
        if (s.end < s.begin) return pce_fail(c, PCE_E_INVALID, "slice %d: end < begin", i);
        const int64_t nx = s.end - s.begin;
        InPlan pl; pl.n_frames = 0; pl.t1 = 0.0;
        const int st = nx == 0 ? PCE_SLICE_EMPTY : intensity_plan_make(nx, dx, s.x1, p, &pl);
        status[(size_t)i] = st;
        if (st == PCE_SLICE_OK && pl.n_frames > INT32_MAX) return pce_fail(c, PCE_E_LIMIT, "slice %d: more than 2^31 - 1 intensity frames", i);
        if (st == PCE_SLICE_OK) t1[(size_t)i] = pl.t1;
        frame_off[(size_t)i + 1] = frame_off[(size_t)i] + (st == PCE_SLICE_OK ? pl.n_frames : 0);
    }
    return PCE_OK;
}

} // namespace

extern "C" {

int pce_intensity_plan(pce_ctx *c, const pce_intensity_params *p, const pce_slice *slices, int32_t n, int64_t *frame_offsets, int32_t *status)
{
    if (!c || !p || (!slices && n > 0) || n < 0 || !frame_offsets) return PCE_E_INVALID;
    if (c->rate <= 0) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    std::vector<int64_t> fo; std::vector<int32_t> st; std::vector<double> t1;
    PCE_TRY(intensity_plan_slices(c, p, slices, n, fo, st, t1));
    memcpy(frame_offsets, fo.data(), sizeof(int64_t) * (size_t)(n + 1));
    if (status && n > 0) memcpy(status, st.data(), sizeof(int32_t) * (size_t)n);
    return PCE_OK;
}

int pce_intensity_run(pce_ctx *c, const pce_intensity_params *p, const double *taps, int32_t n_taps, const pce_slice *slices, int32_t n)
{
    if (!c || !p || !taps || (!slices && n > 0) || n < 0) return PCE_E_INVALID;
    if (!c->d_pcm) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    PCE_HIP(c, hipSetDevice(c->device));
    const bool same = c->in_cache.same(slices, n) && c->in_params_valid && memcmp(&c->in_params, p, sizeof *p) == 0 &&
                      c->in_taps_host.size() == (size_t)(n_taps > 0 ? n_taps : 0) &&
                      (n_taps <= 0 || memcmp(c->in_taps_host.data(), taps, sizeof(double) * (size_t)n_taps) == 0);
    if (!same) {
        c->in_n = -1; c->in_params_valid = false; c->in_cache.drop();
        PCE_TRY(intensity_plan_slices(c, p, slices, n, c->in_frame_off, c->in_status, c->in_t1));
        const double dx = 1.0 / (double)c->rate;
        const double window = 6.4 / p->pitch_floor, half = 0.5 * window;
        const double dt = p->time_step <= 0.0 ? 0.8 / p->pitch_floor : p->time_step;
        const double hs_d = std::floor(half / dx);
        if (2.0 * hs_d + 1.0 > (double)IN_MAX_TAPS)
            return pce_fail(c, PCE_E_LIMIT, "intensity: a window of %.0f taps (pitch floor %g Hz at %d Hz) exceeds the %d the kernel holds "
                            "(pitch floor >= 50 Hz at 48 kHz)", 2.0 * hs_d + 1.0, p->pitch_floor, (int)c->rate, IN_MAX_TAPS);
        const int hs = (int)hs_d;
        if (n_taps != 2 * hs + 1) return pce_fail(c, PCE_E_INVALID, "intensity: %d taps given, the window has %d", (int)n_taps, 2 * hs + 1);
        // frames per workgroup: as many as IN_FPB whose samples fit the staging area (centres of a run of f frames lie within
        // (f - 1) dt / dx + 1 samples of each other)
        int fpb = IN_FPB;
        auto span_of = [&](int f) { return std::ceil((double)(f - 1) * dt / dx) + (double)n_taps + 4.0; };
        while (fpb > 1 && span_of(fpb) > (double)IN_MAX_SPAN) fpb >>= 1;
        const int span = ((int)span_of(fpb) + 7) & ~7;
        c->in_hs = hs; c->in_fpb = fpb; c->in_span = span; c->in_dt = dt;
        c->in_lds = sizeof(double) * (size_t)((n_taps + 1) & ~1) + sizeof(int16_t) * (size_t)(span + 8);

        std::vector<InSlice> meta((size_t)(n > 0 ? n : 1));
        std::vector<InWork> work;
        for (int32_t i = 0; i < n; i++) {
            const pce_slice &s = slices[i];
            InSlice &m = meta[(size_t)i];
            m.begin = s.begin; m.clip_len = c->clip_off[(size_t)s.clip + 1] - c->clip_off[(size_t)s.clip]; m.clip_off = c->clip_off[(size_t)s.clip];
            m.nx = s.end - s.begin; m.frame_off = c->in_frame_off[(size_t)i]; m.x1 = s.x1; m.t1 = c->in_t1[(size_t)i];
            m.n_frames = (int32_t)(c->in_frame_off[(size_t)i + 1] - c->in_frame_off[(size_t)i]); m.status = c->in_status[(size_t)i];
            for (int32_t f = 0; f < m.n_frames; f += fpb) work.push_back({i, f});
        }
        const int64_t total = c->in_frame_off[(size_t)n];
        PCE_HIP(c, c->in_out.reserve(sizeof(double) * (size_t)(total > 0 ? total : 1)));
        PCE_HIP(c, c->in_summary.reserve(sizeof(InSummaryDev) * meta.size()));
        PCE_UPLOAD(c, c->in_meta, meta); PCE_UPLOAD(c, c->in_work, work, 1); PCE_UPLOAD(c, c->in_taps, taps, (size_t)n_taps);
        PCE_HIP(c, hipStreamSynchronize(c->stream));             // the sources are pageable and die at return
        c->in_n_work = (int64_t)work.size();
        c->in_total_frames = total;
        c->in_taps_host.assign(taps, taps + n_taps);
        c->in_params = *p; c->in_params_valid = true;
        c->in_cache.store(slices, n);
        PCE_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_intensity), hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->in_lds));
    }
    InParams P;
    P.dx = 1.0 / (double)c->rate; P.dt = c->in_dt; P.hs = c->in_hs; P.fpb = c->in_fpb; P.span = c->in_span; P.subtract_mean = p->subtract_mean ? 1 : 0;
    if (c->in_n_work > 0) {
        KernelTimer t(c, PCE_K_INTENSITY);
        hipLaunchKernelGGL(k_intensity, dim3((unsigned)c->in_n_work), dim3(IN_THREADS), c->in_lds, c->stream, c->d_pcm, c->in_meta.as<InSlice>(),
                           c->in_work.as<InWork>(), c->in_taps.as<double>(), P, c->in_out.as<double>());
        PCE_HIP(c, hipGetLastError());
    }
    if (n > 0) {
        KernelTimer t(c, PCE_K_INTENSITY_SUMMARY);
        hipLaunchKernelGGL(k_intensity_summary, dim3((unsigned)n), dim3(64), 0, c->stream, c->in_meta.as<InSlice>(), c->in_out.as<double>(),
                           c->in_summary.as<InSummaryDev>());
        PCE_HIP(c, hipGetLastError());
    }
    c->in_n = n;
    return PCE_OK;
}

int pce_intensity_fetch(pce_ctx *c, double *values, pce_intensity_summary *summary)
{
    if (!c) return PCE_E_INVALID;
    if (c->in_n < 0) return pce_fail(c, PCE_E_STATE, "pce_intensity_fetch before pce_intensity_run");
    PCE_HIP(c, hipSetDevice(c->device));
    const int32_t n = c->in_n;
    const int64_t total = c->in_total_frames;
    std::vector<InSummaryDev> sd((size_t)(n > 0 ? n : 1));
    if (values && total > 0) PCE_FETCH(c, values, c->in_out.p, (size_t)total);
    if (summary && n > 0) PCE_FETCH(c, sd.data(), c->in_summary.p, (size_t)n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    if (summary)
        for (int32_t i = 0; i < n; i++) {
            pce_intensity_summary &o = summary[i];
            o.n_frames = c->in_frame_off[(size_t)i + 1] - c->in_frame_off[(size_t)i];
            o.n_positive = sd[(size_t)i].n_positive; o.mean_positive = sd[(size_t)i].mean_positive;
            o.t1 = c->in_t1[(size_t)i]; o.status = c->in_status[(size_t)i]; o.reserved = 0;
        }
    return PCE_OK;
}

} // extern "C"
