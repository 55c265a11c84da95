// pce_pitch.hip -- Praat autocorrelation pitch (R1/R2) on gfx950: the C API and its two host steps.
//
// Replaces parselmouth Sound.to_pitch(pitch_floor, pitch_ceiling) + selected_array +
// voiced median / geometric mean (Code/audioPipeline.py:326-335,
// Code/Pipeline/compute_pitch_adjustments.py:167-208), i.e. Praat's
// Sound_to_Pitch_ac (AC_HANNING) and Pitch_pathFinder.  The published algorithm is
// restated in oracle/pce_oracle.c; this file set is its MI355X execution plan:
//
//   k_energy (shared)     per-slice integer sum / min / max -> global mean and peak (pce_energy.hip; reused when
//                         pce_energy_run has just produced them for the same slices)
//   k_pitch_frames        one wavefront per analysis frame (two at N = 512).  The samples under a work item's
//                         frames are staged in LDS once per workgroup; each frame is mean-subtracted and
//                         Hann-windowed in fp64 and its autocorrelation taken by FFT, as Praat does: forward
//                         transform, power spectrum, the same transform again, division by the window's
//                         autocorrelation.  Four transform forms, chosen by N = nsampFFT (pce_pitch_plan.h):
//                         Stockham passes between two LDS buffers for any N (MODE 0, at 4, 2 or 1 wavefronts per
//                         workgroup as the buffers fit), and register-resident transforms with one LDS exchange
//                         buffer for N = 1024 (MODE 1), N = 512 on half a wavefront (MODE 2, tables in LDS) and
//                         N = 2048 (MODE 3).  Local maxima of r are found with a ballot; their lags and r[0..bix]
//                         go to global memory for the refinement.  Only the rare frame with more maxima than
//                         candidate slots interpolates here (sinc_wave, depth 30, Praat's replacement rule).
//   k_pitch_refine        Praat's second pass (NUMimproveMaximum, sinc depth 70 / 700) over the flat lists of
//                         candidates of all frames, eight lanes per candidate: a seeded parabolic search, Praat's
//                         own Brent iterates where the two could differ (or for all: PCE_PITCH_REFINE=praat).
//   k_pitch_delta         elementwise pre-pass of Pitch_pathFinder: local terms and log2 f per candidate; frames with
//                         the voiceless candidate alone are cuts and get their result here, run starts are listed.
//   k_pitch_path          Viterbi over one run of multi-candidate frames per wavefront (lane = current candidate,
//                         the previous frame's state in registers), back-pointers in LDS, long runs through global tiles.
//   k_pitch_median        one workgroup per slice: bitonic sort of the voiced F0 in LDS; k_pitch_median_long takes
//                         the slices that do not fit by radix selection in global memory.
//
// Files:  pce_pitch_plan.h      host only: Praat's sizes, PiParams, tables, the k_pitch_frames launch, slice table and
//                               work list, buffer sizes; the kernel-argument structs and shared constants
//         pce_pitch_fft.inc     fft_wave, fft256_half / fft512_reg / fft1024_reg, dft4 / 8 / 16, rcp_f64, cmul_f64, wave_sync
//         pce_pitch_frames.inc  sinc_wave, k_pitch_frames
//         pce_pitch_refine.inc  polynomial trigonometry, sinc_group_reg / _mem, k_pitch_refine
//         pce_pitch_path.inc    k_pitch_delta, k_pitch_path, k_pitch_median, k_pitch_median_long
// All of them are this one translation unit.
//
// Roofline: k_pitch_frames is fp64-VALU / LDS bound (about 10^3 flop per algorithmic
// byte), not HBM bound: algorithmic traffic is 2 B of PCM per
// sample plus 8 B of F0 per frame.
#include "pce_internal.h"
#include "pce_wave.h"
#include <cmath>
#include <cstdlib>

namespace {

constexpr double LOG2E_D = 1.4426950408889634073599246810018921374266;

#include "pce_pitch_fft.inc"
#include "pce_pitch_frames.inc"
#include "pce_pitch_refine.inc"
#include "pce_pitch_path.inc"

bool same_params(const pce_pitch_params &a, const pce_pitch_params &b) { return memcmp(&a, &b, sizeof a) == 0; }

// the one place that names the k_pitch_frames instantiations
using FramesKernel = decltype(&k_pitch_frames<4, 0, false>);
FramesKernel frames_kernel(PitchFramesKernel k)
{
    switch (k) {
    case PF_W4_M1: return k_pitch_frames<4, 1, false>;
    case PF_W4_M2_TABS: return k_pitch_frames<4, 2, true>;
    case PF_W4_M3: return k_pitch_frames<4, 3, false>;
    case PF_W4_M0: return k_pitch_frames<4, 0, false>;
    case PF_W2_M0: return k_pitch_frames<2, 0, false>;
    case PF_W1_M0: return k_pitch_frames<1, 0, false>;
    }
    return nullptr;
}

int plan_slices(pce_ctx *c, const pce_pitch_params *p, const pce_slice *slices, int32_t n,
                std::vector<int64_t> &frame_off, std::vector<int32_t> &status, std::vector<double> &t1, PitchPlan *common)
{
    int why = 0;
    const int32_t bad = pitch_plan_slices(c->rate, c->n_clips, p, slices, n, frame_off, status, t1, common, &why);
    if (bad >= 0 && why == 1) return pce_fail(c, PCE_E_INVALID, "slice %d: clip %d out of range", bad, slices[bad].clip);
    if (bad >= 0) return pce_fail(c, PCE_E_INVALID, "slice %d: end < begin", bad);
    return PCE_OK;
}

// cache miss: the plan of pce_pitch_plan.h for this slice list and these parameters, uploaded, and room for everything the launches write
int pitch_prepare(pce_ctx *c, const pce_pitch_params *p, const pce_slice *slices, int32_t n)
{
    c->pi_n = -1; c->pi_params_valid = false;
    PitchPlan pl;
    PCE_TRY(plan_slices(c, p, slices, n, c->pi_frame_off, c->pi_status, c->pi_t1, &pl));
    const int64_t total = c->pi_frame_off[(size_t)n];
    c->pi_total_frames = total;
    PiParams P; memset(&P, 0, sizeof P);
    if (total > 0) {
        const PitchParamsStatus st = pitch_params_make(c->rate, p, pl, c->pitch_refine_praat, &P);
        if (st == PITCH_PARAMS_CANDIDATES) return pce_fail(c, PCE_E_LIMIT, "more than %d pitch candidates per frame requested", PI_MAXC);
        if (st == PITCH_PARAMS_LDS) return pce_fail(c, PCE_E_LIMIT, "analysis window of %d samples does not fit LDS", P.nw);
        PitchTables t;
        pitch_tables_make(pl, P, t);
        PCE_UPLOAD(c, c->pi_tw, t.tw);
        PCE_UPLOAD(c, c->pi_window, t.window);
        PCE_UPLOAD(c, c->pi_windowR, t.windowR);
        if (P.mode != 0) PCE_UPLOAD(c, c->pi_blob, t.blob);
        PCE_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->pi_P = P;
    PitchWork w;
    pitch_work_make(slices, n, c->clip_off, c->pi_frame_off, c->pi_status, c->pi_t1, P.fpb, w);
    if (w.too_many >= 0) return pce_fail(c, PCE_E_LIMIT, "slice %d has too many frames", w.too_many);
    c->pi_np2 = w.np2;
    c->pi_long_slices = w.long_slices;
    c->pi_n_work = (int64_t)w.work.size();
    c->pi_launch = pitch_frames_launch(P, c->pi_n_work);
    const PitchSizes z = c->pi_sizes = pitch_sizes(P, total, c->pi_n_work, w.slices.size());
    PCE_HIP(c, c->pi_cand.reserve(z.cand));
    PCE_HIP(c, c->pi_gpeak.reserve(z.gpeak));
    PCE_HIP(c, c->pi_psi.reserve(z.psi));
    PCE_HIP(c, c->pi_f0.reserve(z.f0));
    PCE_HIP(c, c->pi_strength.reserve(z.strength));
    PCE_HIP(c, c->pi_summary.reserve(z.summary));
    PCE_HIP(c, c->pi_runs.reserve(z.runs));
    PCE_HIP(c, c->pi_dl.reserve(z.dl));
    PCE_HIP(c, c->pi_rr.reserve(z.rr));
    PCE_HIP(c, c->pi_items.reserve(z.items));
    PCE_UPLOAD(c, c->pi_meta, w.slices);
    PCE_UPLOAD(c, c->pi_work, w.work, 1);
    PCE_UPLOAD(c, c->pi_fslice, w.frame_slice);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    PCE_TRY(pce_energy_plan(c, slices, n, c->pi_peakwork, c->pi_acc, &c->pi_n_energy_work));
    c->pi_cache.store(slices, n);
    c->pi_params = *p; c->pi_params_valid = true;
    return PCE_OK;
}

// the launches behind the refinement: local terms, path finder and voiced summaries of `n` slices, from the candidates, counts and intensities
// in the pitch buffers and the plan in the context (pi_P, pi_sizes, pi_total_frames, pi_np2, pi_long_slices, pi_meta, pi_fslice).
// pitch_launch and pce_selftest_pitch_path both end here: there is no other launch of these four kernels.
int pitch_launch_tail(pce_ctx *c, int32_t n)
{
    const PiParams &P = c->pi_P;
    const PitchSizes &z = c->pi_sizes;
    hipStream_t tail = c->stream;
    const int64_t total = c->pi_total_frames;
    if (total > 0) {
        double *intensity = c->pi_gpeak.as<double>();
        int *ncand = reinterpret_cast<int *>(intensity + (total + 1));
        unsigned int *run_count = c->pi_runs.as<unsigned int>();
        PathRun *runs = reinterpret_cast<PathRun *>(c->pi_runs.as<char>() + z.run_count_bytes);
        // everything after the refinement (local terms, path finder, median) goes to the side stream: it is HBM- and
        // latency-bound, and whatever the caller launches next on the main stream runs beside it; every consumer
        // joins first (pce_side_join)
        { int rc2 = pce_side_begin(c, pce_ctx::SIDE_TAIL, &tail); if (rc2) return rc2; }
        PCE_HIP(c, hipMemsetAsync(run_count, 0, z.run_count_bytes, tail));
        const long long ne = total * PI_MAXC;
        {
            KernelTimer t(c, PCE_K_PITCH_DELTA, tail);
            hipLaunchKernelGGL(k_pitch_delta, dim3((unsigned)div_up(ne, 256)), dim3(256), 0, tail, P, c->pi_meta.as<PiSlice>(),
                               c->pi_fslice.as<int>(), c->pi_cand.as<double>(), ncand, intensity, (long long)total,
                               c->pi_dl.as<double2>(), c->pi_f0.as<double>(), c->pi_strength.as<double>(), runs, run_count, z.run_cap);
        }
        {
            KernelTimer t(c, PCE_K_PITCH_PATH, tail);
            const unsigned blocks = (unsigned)(c->cu_count > 0 ? c->cu_count : 256) * 16u;     // multiple of RUN_LISTS
            hipLaunchKernelGGL(k_pitch_path, dim3(blocks), dim3(64), 0, tail, P,
                               c->pi_cand.as<double>(), ncand, c->pi_dl.as<double2>(), runs, run_count, z.run_cap,
                               c->pi_psi.as<unsigned char>(), c->pi_f0.as<double>(), c->pi_strength.as<double>());
        }
    }
    if (n > 0) {
        const size_t lds = sizeof(double) * (size_t)c->pi_np2;
        if (lds > 64 * 1024)
            PCE_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_pitch_median), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        KernelTimer t(c, PCE_K_PITCH_MEDIAN, tail);
        hipLaunchKernelGGL(k_pitch_median, dim3((unsigned)n), dim3(256), lds, tail, c->pi_meta.as<PiSlice>(),
                           c->pi_f0.as<double>(), c->pi_np2, c->pi_summary.as<PiSummaryDev>());
        if (c->pi_long_slices)
            hipLaunchKernelGGL(k_pitch_median_long, dim3((unsigned)n), dim3(256), 0, tail, c->pi_meta.as<PiSlice>(), c->pi_f0.as<double>(), c->pi_np2,
                               c->pi_summary.as<PiSummaryDev>());
    }
    { int rc2 = pce_side_end(c, pce_ctx::SIDE_TAIL, tail); if (rc2) return rc2; }
    PCE_HIP(c, hipGetLastError());
    return PCE_OK;
}

// the launches of one run, from what pitch_prepare left in the context
int pitch_launch(pce_ctx *c, const pce_slice *slices, int32_t n)
{
    const PiParams &P = c->pi_P;
    const PitchSizes &z = c->pi_sizes;
    const int64_t total = c->pi_total_frames;
    if (total > 0) {
        // the slice sums and extrema (Praat's mean subtraction and global peak): when pce_energy_run has just produced them
        // for this very slice list they are read from its accumulators (stream ordered) instead of streaming the batch again
        const bool reuse = c->en_n == n && c->en_cache.same(slices, n);
        if (!reuse) {
            PCE_TRY(pce_energy_launch(c, n, 500, c->pi_n_energy_work, c->pi_peakwork, c->pi_acc));
        }
        size_t stride; const long long *a_sum; const int *a_hi, *a_lo;
        pce_energy_range_ptrs(reuse ? c->en_out : c->pi_acc, &stride, &a_sum, &a_hi, &a_lo);
        double *intensity = c->pi_gpeak.as<double>();
        int *ncand = reinterpret_cast<int *>(intensity + (total + 1));
        {
            const PitchFramesLaunch &fl = c->pi_launch;
            const FramesKernel kern = frames_kernel(fl.kernel);
            if (fl.lds > 64 * 1024)
                PCE_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl.lds));
            RefineItem *items = reinterpret_cast<RefineItem *>(c->pi_items.as<char>() + z.item_count_bytes);
            unsigned int *item_count = c->pi_items.as<unsigned int>();
            PCE_HIP(c, hipMemsetAsync(item_count, 0, z.item_count_bytes, c->stream));
            {
                // algorithmic fp64 work of a frame (Praat's formulation): mean removal + window (3 nw), two real FFTs of nfft points
                // (2.5 nfft log2 nfft each), the power spectrum (3 nfft / 2), the window-autocorrelation division (maxlag)
                const double f_flops = 3.0 * P.nw + 5.0 * P.nfft * std::log2((double)P.nfft) + 1.5 * P.nfft + (double)P.maxlag;
                KernelTimer t(c, PCE_K_PITCH_FRAMES, nullptr, f_flops * (double)total);
                hipLaunchKernelGGL(kern, dim3((unsigned)fl.grid), dim3(64 * fl.wpb), fl.lds, c->stream, c->d_pcm,
                                   c->pi_meta.as<PiSlice>(), c->pi_work.as<PiWork>(), (int)c->pi_n_work, P,
                                   c->pi_window.as<double>(), c->pi_windowR.as<double>(), c->pi_tw.as<double2>(),
                                   c->pi_tw.as<double2>() + (P.nfft >> 1), a_sum, a_hi, a_lo, stride,
                                   c->pi_cand.as<double>(), ncand, intensity, c->pi_rr.as<double>(), items, item_count, z.list_cap,
                                   c->pi_blob.as<double>());
            }
            {
                KernelTimer t(c, PCE_K_PITCH_REFINE);
                // 12 wavefronts per CU are resident (168 VGPRs); 96 per CU measured best (the lists and the iteration counts are uneven), as
                // ONE-wavefront workgroups: a slot is free again when its wavefront ends, not when the slowest of four does (0.98 -> 0.89-0.93 ms).
                // Tried and dropped in round 3: 4 or 16 lanes per candidate (1.66 / 1.02 ms against 0.98); the refinement inside
                // k_pitch_frames, on the autocorrelation still in LDS (no hand-off through HBM: -700 MB per C2 step): 3.07 ms for the
                // fused kernel against 0.95 + 0.98 -- a wavefront's two frames hold ~11 candidates, so its eight lane groups run two rounds of
                // 3-4 dependent evaluations at 70 % occupancy of the lanes, serialised behind its own transforms, where this kernel packs
                // eight candidates of any frames into every wavefront.
                const unsigned blocks = (unsigned)(c->cu_count > 0 ? c->cu_count : 256) * 96u;
                hipLaunchKernelGGL(k_pitch_refine<8>, dim3(blocks), dim3(64), 0, c->stream, P, c->pi_rr.as<double>(), items, item_count,
                                   z.list_cap, c->pi_cand.as<double>());
            }
        }
    }
    return pitch_launch_tail(c, n);
}

} // namespace

// ---------------------------------------------------------------------------
// host API
// ---------------------------------------------------------------------------
extern "C" {

int pce_pitch_plan(pce_ctx *c, const pce_pitch_params *p, const pce_slice *slices, int32_t n, int64_t *frame_offsets, int32_t *status)
{
    if (!c || !p || (!slices && n > 0) || n < 0 || !frame_offsets) return PCE_E_INVALID;
    if (c->rate <= 0) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    std::vector<int64_t> fo; std::vector<int32_t> st; std::vector<double> t1; PitchPlan common;
    PCE_TRY(plan_slices(c, p, slices, n, fo, st, t1, &common));
    memcpy(frame_offsets, fo.data(), sizeof(int64_t) * (size_t)(n + 1));
    if (status) memcpy(status, st.data(), sizeof(int32_t) * (size_t)n);
    return PCE_OK;
}

int pce_pitch_set_refine(pce_ctx *c, int32_t mode)
{
    if (!c || (mode != PCE_REFINE_SEEDED && mode != PCE_REFINE_PRAAT)) return PCE_E_INVALID;
    const bool praat = mode == PCE_REFINE_PRAAT;
    if (c->pitch_refine_praat != praat) { c->pitch_refine_praat = praat; c->pi_cache.drop(); c->pi_params_valid = false; }
    return PCE_OK;
}

int pce_pitch_run(pce_ctx *c, const pce_pitch_params *p, const pce_slice *slices, int32_t n)
{
    if (!c || !p || (!slices && n > 0) || n < 0) return PCE_E_INVALID;
    if (!c->d_pcm) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(pce_side_join(c, pce_ctx::SIDE_TAIL));   // the previous run's tail still owns the pitch buffers
    if (!(c->pi_cache.same(slices, n) && c->pi_params_valid && same_params(c->pi_params, *p))) PCE_TRY(pitch_prepare(c, p, slices, n));
    PCE_TRY(pitch_launch(c, slices, n));
    c->pi_n = n;
    return PCE_OK;
}

int pce_pitch_fetch(pce_ctx *c, double *f0, double *strength, pce_pitch_summary *summary)
{
    if (!c) return PCE_E_INVALID;
    if (c->pi_n < 0) return pce_fail(c, PCE_E_STATE, "pce_pitch_fetch before pce_pitch_run");
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(pce_side_join(c, pce_ctx::SIDE_TAIL));
    const int32_t n = c->pi_n;
    const int64_t total = c->pi_total_frames;
    std::vector<PiSummaryDev> sd((size_t)(n > 0 ? n : 1));
    if (f0 && total > 0) PCE_FETCH(c, f0, c->pi_f0.p, (size_t)total);
    if (strength && total > 0) PCE_FETCH(c, strength, c->pi_strength.p, (size_t)total);
    if (summary && n > 0) PCE_FETCH(c, sd.data(), c->pi_summary.p, (size_t)n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    if (summary)
        for (int32_t i = 0; i < n; i++) {
            pce_pitch_summary &o = summary[i];
            o.n_frames = c->pi_frame_off[(size_t)i + 1] - c->pi_frame_off[(size_t)i];
            o.n_voiced = sd[(size_t)i].n_voiced; o.median_f0 = sd[(size_t)i].median; o.mean_log_f0 = sd[(size_t)i].mean_log;
            o.t1 = c->pi_t1[(size_t)i]; o.status = c->pi_status[(size_t)i]; o.reserved = 0;
        }
    return PCE_OK;
}

int pce_pitch_fetch_candidates(pce_ctx *c, int32_t *ncand, double *intensity, double *cand_f, double *cand_s)
{
    if (!c) return PCE_E_INVALID;
    if (c->pi_n < 0) return pce_fail(c, PCE_E_STATE, "pce_pitch_fetch_candidates before pce_pitch_run");
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(pce_side_join(c, pce_ctx::SIDE_TAIL));
    const int64_t total = c->pi_total_frames;
    if (total <= 0) return PCE_OK;
    std::vector<int32_t> n((size_t)total);
    std::vector<double> img((cand_f || cand_s) ? (size_t)total * 32 : 0);
    const double *d_int = c->pi_gpeak.as<double>();
    PCE_FETCH(c, n.data(), d_int + (total + 1), (size_t)total);
    if (intensity) PCE_FETCH(c, intensity, d_int, (size_t)total);
    if (!img.empty()) PCE_FETCH(c, img.data(), c->pi_cand.p, img.size());
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    for (int64_t f = 0; f < total; f++) {
        if (ncand) ncand[f] = n[(size_t)f];
        // slot 0 is the voiceless candidate by definition; slots >= ncand were never written: the caller's prefill stays
        const int live = n[(size_t)f] < PI_MAXC ? n[(size_t)f] : PI_MAXC;
        for (int j = 0; j < live; j++) {
            if (cand_f) cand_f[f * PI_MAXC + j] = j ? img[(size_t)f * 32 + (size_t)j] : 0.0;
            if (cand_s) cand_s[f * PI_MAXC + j] = j ? img[(size_t)f * 32 + 16 + (size_t)j] : 0.0;
        }
    }
    return PCE_OK;
}

int pce_selftest_pitch_path(pce_ctx *c, const pce_pitch_params *p, double dt, int32_t n_slices, const int64_t *frame_off, const int32_t *ncand,
                            const double *intensity, const double *cand_f, const double *cand_s, double *f0, double *strength, uint8_t *psi,
                            pce_pitch_summary *summary)
{
    if (!c || !p || !frame_off || !ncand || !intensity || !cand_f || !cand_s) return PCE_E_INVALID;
    if (n_slices < 1 || n_slices > (1 << 20) || frame_off[0] != 0) return pce_fail(c, PCE_E_INVALID, "pce_selftest_pitch_path: 1 .. 2^20 slices, frame_off[0] == 0");
    for (int32_t i = 0; i < n_slices; i++)
        if (frame_off[i + 1] < frame_off[i]) return pce_fail(c, PCE_E_INVALID, "pce_selftest_pitch_path: frame_off decreases at slice %d", i);
    const int64_t total = frame_off[n_slices];
    if (total < 1 || total > (int64_t)1 << 24) return pce_fail(c, PCE_E_INVALID, "pce_selftest_pitch_path: 1 .. 2^24 frames");
    if (!(dt > 0.0)) return pce_fail(c, PCE_E_INVALID, "pce_selftest_pitch_path: dt must be positive");
    if (p->max_candidates > PI_MAXC) return pce_fail(c, PCE_E_LIMIT, "more than %d pitch candidates per frame requested", PI_MAXC);
    for (int64_t f = 0; f < total; f++)
        if (ncand[f] < 1 || ncand[f] > PI_MAXC) return pce_fail(c, PCE_E_INVALID, "pce_selftest_pitch_path: frame %lld has %d candidates", (long long)f, ncand[f]);
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_TRY(pce_side_join(c, pce_ctx::SIDE_TAIL));
    c->pi_cache.drop(); c->pi_n = -1; c->pi_params_valid = false;   // the pitch buffers and the plan in the context are this call's from here on

    PiParams P; memset(&P, 0, sizeof P);
    P.dt = dt; P.min_pitch = p->pitch_floor; P.ceiling = p->pitch_ceiling;    // the ceiling as given: no clamp to the Nyquist frequency without a rate
    P.voicing_thr = p->voicing_threshold; P.octave_cost = p->octave_cost; P.silence_thr = p->silence_threshold;
    P.oj_cost = p->octave_jump_cost; P.vuv_cost = p->voiced_unvoiced_cost;
    P.maxc = p->max_candidates < 2 ? 2 : p->max_candidates; P.fpb = PI_FPB;
    // the slice table, frame -> slice table and median plan of a real run over slices of these frame counts (no samples behind them)
    std::vector<pce_slice> sl((size_t)n_slices);
    memset(sl.data(), 0, sizeof(pce_slice) * sl.size());
    const std::vector<int64_t> clip_off{0, 0}, fo(frame_off, frame_off + n_slices + 1);
    const std::vector<int32_t> status((size_t)n_slices, PCE_SLICE_OK);
    const std::vector<double> t1((size_t)n_slices, 0.0);
    PitchWork w;
    pitch_work_make(sl.data(), n_slices, clip_off, fo, status, t1, P.fpb, w);
    if (w.too_many >= 0) return pce_fail(c, PCE_E_LIMIT, "slice %d has too many frames", w.too_many);
    c->pi_P = P; c->pi_total_frames = total; c->pi_np2 = w.np2; c->pi_long_slices = w.long_slices;
    c->pi_n_work = (int64_t)w.work.size();
    const PitchSizes z = c->pi_sizes = pitch_sizes(P, total, c->pi_n_work, w.slices.size());
    PCE_HIP(c, c->pi_cand.reserve(z.cand));
    PCE_HIP(c, c->pi_gpeak.reserve(z.gpeak));
    PCE_HIP(c, c->pi_psi.reserve(z.psi));
    PCE_HIP(c, c->pi_f0.reserve(z.f0));
    PCE_HIP(c, c->pi_strength.reserve(z.strength));
    PCE_HIP(c, c->pi_summary.reserve(z.summary));
    PCE_HIP(c, c->pi_runs.reserve(z.runs));
    PCE_HIP(c, c->pi_dl.reserve(z.dl));
    PCE_UPLOAD(c, c->pi_meta, w.slices);
    PCE_UPLOAD(c, c->pi_fslice, w.frame_slice);
    // the device layout of the candidates: [frames][32], strengths at + 16
    std::vector<double> img((size_t)total * 32, 0.0);
    for (int64_t f = 0; f < total; f++)
        for (int j = 0; j < PI_MAXC; j++) {
            img[(size_t)f * 32 + (size_t)j] = cand_f[f * PI_MAXC + j];
            img[(size_t)f * 32 + 16 + (size_t)j] = cand_s[f * PI_MAXC + j];
        }
    double *d_int = c->pi_gpeak.as<double>();
    PCE_PUT(c, c->pi_cand.p, img.data(), img.size());
    PCE_PUT(c, static_cast<void *>(d_int), intensity, (size_t)total);
    PCE_PUT(c, static_cast<void *>(d_int + (total + 1)), ncand, (size_t)total);
    PCE_HIP(c, hipMemsetAsync(c->pi_psi.p, 0, z.psi, c->stream));   // cut frames have no back-pointers: they read 0
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    PCE_TRY(pitch_launch_tail(c, n_slices));
    PCE_TRY(pce_side_join(c, pce_ctx::SIDE_TAIL));
    std::vector<PiSummaryDev> sd((size_t)n_slices);
    if (f0) PCE_FETCH(c, f0, c->pi_f0.p, (size_t)total);
    if (strength) PCE_FETCH(c, strength, c->pi_strength.p, (size_t)total);
    if (psi) PCE_FETCH(c, psi, c->pi_psi.p, (size_t)total * PI_MAXC);
    if (summary) PCE_FETCH(c, sd.data(), c->pi_summary.p, (size_t)n_slices);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    if (summary)
        for (int32_t i = 0; i < n_slices; i++) {
            pce_pitch_summary &o = summary[i];
            o.n_frames = frame_off[i + 1] - frame_off[i];
            o.n_voiced = sd[(size_t)i].n_voiced; o.median_f0 = sd[(size_t)i].median; o.mean_log_f0 = sd[(size_t)i].mean_log;
            o.t1 = 0.0; o.status = PCE_SLICE_OK; o.reserved = 0;
        }
    return PCE_OK;
}

} // extern "C"

size_t pce_pitch_stage_bytes(const pce_ctx *c) { return c->pi_n > 0 ? sizeof(PiSummaryDev) * (size_t)c->pi_n : 0; }
int pce_pitch_stage_enqueue(pce_ctx *c, void *pinned, hipStream_t on)
{
    if (c->pi_n > 0)
        PCE_HIP(c, hipMemcpyAsync(pinned, c->pi_summary.p, sizeof(PiSummaryDev) * (size_t)c->pi_n, hipMemcpyDeviceToHost, on ? on : c->stream));
    return PCE_OK;
}
void pce_pitch_stage_unpack(const void *pinned, int32_t n, pce_pitch_summary *out)
{
    const PiSummaryDev *sd = static_cast<const PiSummaryDev *>(pinned);
    for (int32_t i = 0; i < n; i++) { out[i].n_voiced = sd[i].n_voiced; out[i].median_f0 = sd[i].median; out[i].mean_log_f0 = sd[i].mean_log; }
}
