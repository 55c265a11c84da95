// pce_pitch_plan.h -- the host plan of the Praat autocorrelation pitch path (pce_pitch.hip): the sizes Sound_to_Pitch_any derives before its
// frame loop, the kernel parameters and tables made from them, which k_pitch_frames instantiation runs and with what launch, the slice table
// and work list, and the size of every device buffer.  The structs the kernels take as arguments and the constants they share with the host
// live here too.  Host only, no HIP, pure functions over plain structs and vectors: tests/host/pitch_plan_main.cpp builds this file alone
// (with -ffp-contract=off like the library: the index arithmetic below must execute the operation order written).
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include "pce.h"

constexpr double PI_D = 3.1415926535897932384626433832795028841972;
constexpr int PI_WPB = 4;                 // waves per block in k_pitch_frames
constexpr int PI_FPB = 4;                 // frames per work item (one per wave measured fastest: silent frames exit early)
constexpr int PI_MAXC = 16;               // candidates per frame the kernels can hold
constexpr int PI_MEDIAN_LDS = 16384;      // voiced F0 values k_pitch_median sorts in LDS (128 KB)
constexpr int RF_LISTS = 256;             // independent candidate lists (one hot counter would serialise in L2)
constexpr int RF_CSTRIDE = 32;            // counters on their own 128-byte lines
constexpr int RUN_LISTS = 64;             // independent run lists (see RF_LISTS)
constexpr int R_WAVE_F64 = 2 * 8 * 72;    // doubles of LDS per wavefront on the register paths (MODE 1, 2)
constexpr int R3_WAVE_F64 = 2 * 1168;     // ... MODE 3: images [16][72] and [8][129] (+64) complex
constexpr int reg_wave_f64(int mode) { return mode == 3 ? R3_WAVE_F64 : R_WAVE_F64; }
constexpr size_t PI_LDS_LIMIT = 160 * 1024;   // LDS of a CU: what one workgroup of k_pitch_frames may ask for

// ---------------------------------------------------------------------------
// kernel arguments and device tables
// ---------------------------------------------------------------------------
struct PiParams {
    double dx, dt, min_pitch, ceiling, voicing_thr, octave_cost, silence_thr, oj_cost, vuv_cost;
    int nsp, hsp, nw, hw, maxlag, bix, maxc, nfft, zlen, rr_len, mode, fpb;
    int o_tw2, o_twN, o_win, o_winR, blob_f64, pcm_span, tabs, rr_half;   // register paths: table blob layout (offsets in doubles)
    int refine_seeded, pad_;                                              // k_pitch_refine: 1 = parabolic search first (default), 0 = Praat's own iterates for every candidate
    double refine_tol_rel;                                                // ... and the relative step below which the parabolic search stops (3e-8)
};
struct PiSlice {
    int64_t begin, clip_len, clip_off, nx, frame_off;
    double x1, t1;
    int32_t n_frames, status;
};
struct PiWork { int32_t slice, frame0; };
struct RefineItem { long long frame; int slot; int imax; };
struct PathRun { long long frame; long long gend; int has_prev; int pad; };   // run start, slice end (global frame indices), a cut frame precedes
struct PiSummaryDev { long long n_voiced; double median; double mean_log; };

// ---------------------------------------------------------------------------
// the sizes Sound_to_Pitch_any derives before its frame loop
// ---------------------------------------------------------------------------
struct PitchPlan {
    double dt, t1, ceiling, dt_window;
    int64_t n_frames, nsamp_period, halfnsamp_period, nsamp_window, halfnsamp_window;
    int64_t maximum_lag, brent_ixmax, max_candidates;
};
inline int pitch_plan_make(int64_t nx, double dx, double x1, const pce_pitch_params *p, PitchPlan *pl)
{
    double dt = p->time_step, minimumPitch = p->pitch_floor, periodsPerWindow = p->periods_per_window;
    double ceiling = p->pitch_ceiling;
    int64_t maxnCandidates = p->max_candidates;
    if (nx < 1 || !(dx > 0.0) || !(minimumPitch > 0.0) || !(periodsPerWindow > 0.0)) return PCE_SLICE_TOO_SHORT;
    if (maxnCandidates < 2) maxnCandidates = 2;
    if ((double)maxnCandidates < ceiling / minimumPitch) maxnCandidates = (int64_t)std::floor(ceiling / minimumPitch);
    if (dt <= 0.0) dt = periodsPerWindow / minimumPitch / 4.0;
    const double duration = dx * (double)nx;
    if (minimumPitch < periodsPerWindow / duration) return PCE_SLICE_TOO_SHORT;
    pl->nsamp_period = (int64_t)std::floor(1.0 / dx / minimumPitch);
    pl->halfnsamp_period = pl->nsamp_period / 2 + 1;
    if (ceiling > 0.5 / dx) ceiling = 0.5 / dx;
    pl->dt_window = periodsPerWindow / minimumPitch;
    pl->nsamp_window = (int64_t)std::floor(pl->dt_window / dx);
    pl->halfnsamp_window = pl->nsamp_window / 2 - 1;
    if (pl->halfnsamp_window < 2) return PCE_SLICE_TOO_SHORT;
    pl->nsamp_window = pl->halfnsamp_window * 2;
    pl->maximum_lag = (int64_t)std::floor((double)pl->nsamp_window / periodsPerWindow) + 2;
    if (pl->maximum_lag > pl->nsamp_window) pl->maximum_lag = pl->nsamp_window;
    const double myDuration = dx * (double)nx;
    if (pl->dt_window > myDuration) return PCE_SLICE_TOO_SHORT;
    pl->n_frames = (int64_t)std::floor((myDuration - pl->dt_window) / dt) + 1;
    if (pl->n_frames < 1) return PCE_SLICE_TOO_SHORT;
    const double ourMidTime = x1 - 0.5 * dx + 0.5 * myDuration;
    const double thyDuration = (double)pl->n_frames * dt;
    pl->t1 = ourMidTime - 0.5 * thyDuration + 0.5 * dt;
    pl->dt = dt; pl->ceiling = ceiling; pl->max_candidates = maxnCandidates;
    pl->brent_ixmax = (int64_t)((double)pl->nsamp_window * 0.5);
    return PCE_SLICE_OK;
}

// Every slice of a batch: status, first frame and t1, and the plan of the first analysable one (all zero when none is: those sizes do not
// depend on the slice length).  -> the first slice that cannot be planned at all (*why: 1 = its clip is out of range, 2 = end < begin), else -1.
inline int32_t pitch_plan_slices(int32_t rate, int32_t n_clips, const pce_pitch_params *p, const pce_slice *slices, int32_t n,
                                 std::vector<int64_t> &frame_off, std::vector<int32_t> &status, std::vector<double> &t1, PitchPlan *common, int *why)
{
    const double dx = 1.0 / (double)rate;
    frame_off.assign((size_t)n + 1, 0); status.assign((size_t)n, PCE_SLICE_OK); t1.assign((size_t)n, 0.0);
    bool have = false;
    for (int32_t i = 0; i < n; i++) {
        const pce_slice &s = slices[i];
        if (s.clip < 0 || s.clip >= n_clips) { *why = 1; return i; }
        if (s.end < s.begin) { *why = 2; return i; }
        PitchPlan pl;
        const int64_t nx = s.end - s.begin;
        int st = nx == 0 ? PCE_SLICE_EMPTY : pitch_plan_make(nx, dx, s.x1, p, &pl);
        status[(size_t)i] = st;
        int64_t nf = 0;
        if (st == PCE_SLICE_OK) { nf = pl.n_frames; t1[(size_t)i] = pl.t1; if (!have) { *common = pl; have = true; } }
        frame_off[(size_t)i + 1] = frame_off[(size_t)i] + nf;
    }
    if (!have) memset(common, 0, sizeof *common);
    return -1;
}

// ---------------------------------------------------------------------------
// PiParams: everything but the blob offsets (pitch_tables_make sets those)
// ---------------------------------------------------------------------------
inline size_t pitch_stockham_wave_bytes(int zlen) { return sizeof(double) * 4 * (size_t)zlen; }     // MODE 0: two complex buffers per wavefront

enum PitchParamsStatus {
    PITCH_PARAMS_OK = 0,
    PITCH_PARAMS_CANDIDATES,    // more than PI_MAXC candidates per frame
    PITCH_PARAMS_LDS            // one wavefront's two Stockham buffers exceed the LDS (P->nw, P->zlen are set)
};
inline PitchParamsStatus pitch_params_make(int32_t rate, const pce_pitch_params *p, const PitchPlan &pl, bool refine_praat, PiParams *out)
{
    PiParams &P = *out;
    memset(&P, 0, sizeof P);
    if (pl.max_candidates > PI_MAXC) return PITCH_PARAMS_CANDIDATES;
    P.dx = 1.0 / (double)rate; P.dt = pl.dt; P.min_pitch = p->pitch_floor; P.ceiling = pl.ceiling;
    P.voicing_thr = p->voicing_threshold; P.octave_cost = p->octave_cost; P.silence_thr = p->silence_threshold;
    P.oj_cost = p->octave_jump_cost; P.vuv_cost = p->voiced_unvoiced_cost;
    P.nsp = (int)pl.nsamp_period; P.hsp = (int)pl.halfnsamp_period; P.nw = (int)pl.nsamp_window; P.hw = (int)pl.halfnsamp_window;
    P.maxlag = (int)pl.maximum_lag; P.bix = (int)pl.brent_ixmax; P.maxc = (int)pl.max_candidates;
    int nfft = 8;
    while ((double)nfft < (double)P.nw * 1.5) nfft *= 2;          // Praat's nsampFFT
    P.nfft = nfft;
    const int Mc = nfft / 2;
    P.zlen = Mc + Mc / 8 + 2;
    P.rr_len = 2 * P.bix + 2;
    P.rr_half = (P.bix + 2) & ~1;                  // handoff row: r[0..bix], even length
    P.refine_seeded = refine_praat ? 0 : 1;
    P.refine_tol_rel = 3e-8;
    if (pitch_stockham_wave_bytes(P.zlen) > PI_LDS_LIMIT) return PITCH_PARAMS_LDS;
    // register-resident transforms where N allows it and r[-bix..bix] fits the exchange region
    // (tables stay in global memory: staging them in LDS per workgroup measured slower than L1 hits)
    P.mode = (nfft == 1024 && P.rr_len <= R_WAVE_F64) ? 1
             : (nfft == 512 && P.rr_len <= R_WAVE_F64 / 2) ? 2
             : (nfft == 2048 && P.rr_len <= R3_WAVE_F64) ? 3 : 0;
    P.fpb = P.mode == 2 ? 2 * PI_FPB : PI_FPB;
    P.tabs = P.mode == 2;   // MODE 3: 75 KB of exchange images leave no room
    P.pcm_span = (((int)std::ceil((double)(P.fpb - 1) * P.dt / P.dx) + P.nw + 4) + 7) & ~7;   // samples under one work item's frames
    return PITCH_PARAMS_OK;
}

// ---------------------------------------------------------------------------
// tables
// ---------------------------------------------------------------------------
// Hanning window and its normalised autocorrelation (direct sums, fp64).
inline void make_window_tables(const PitchPlan &pl, std::vector<double> &window, std::vector<double> &windowR)
{
    const int64_t nw = pl.nsamp_window, bix = pl.brent_ixmax;
    window.resize((size_t)nw);
    for (int64_t i = 1; i <= nw; i++) window[(size_t)(i - 1)] = 0.5 - 0.5 * std::cos((double)i * 2.0 * PI_D / (double)(nw + 1));
    windowR.assign((size_t)(bix + 1), 0.0);
    for (int64_t k = 0; k <= bix; k++) {
        long double acc = 0.0L;
        for (int64_t j = 0; j + k < nw; j++) acc += (long double)window[(size_t)j] * (long double)window[(size_t)(j + k)];
        windowR[(size_t)k] = (double)acc;
    }
    const double w0 = windowR[0];
    for (int64_t k = 1; k <= bix; k++) windowR[(size_t)k] /= w0;
    windowR[0] = 1.0;
}

struct PitchTables {
    std::vector<double> tw;                 // twM[m] = exp(-2 pi i m / M), m < M, then twN[k] = exp(-2 pi i k / N), k <= M (re, im pairs)
    std::vector<double> window, windowR;    // [nw], [bix + 1]
    std::vector<double> blob;               // register paths only: the lane-ordered image below
};
// Fills the tables for P (as pitch_params_make left it) and P's blob offsets.
inline void pitch_tables_make(const PitchPlan &pl, PiParams &P, PitchTables &t)
{
    const int nfft = P.nfft, Mc = nfft / 2;
    std::vector<double> &tw = t.tw;
    tw.assign((size_t)(Mc + Mc + 1) * 2, 0.0);
    for (int m = 0; m < Mc; m++) { tw[2 * (size_t)m] = std::cos(2.0 * PI_D * m / Mc); tw[2 * (size_t)m + 1] = -std::sin(2.0 * PI_D * m / Mc); }
    for (int k = 0; k <= Mc; k++) { tw[2 * (size_t)(Mc + k)] = std::cos(2.0 * PI_D * k / nfft); tw[2 * (size_t)(Mc + k) + 1] = -std::sin(2.0 * PI_D * k / nfft); }
    make_window_tables(pl, t.window, t.windowR);
    std::vector<double> &blob = t.blob;
    blob.clear();
    if (P.mode != 0) {
        // lane-ordered tables for the register paths: tw1[k-1][l] = W_M^(l k), tw2[k-1][c] = W_M^(8 c k),
        // twN[k] = W_N^k (k < M), window, windowR[0..bix]; every table starts on a 16-byte boundary
        const int LW = P.mode == 2 ? 32 : 64, CW = LW / 8, NK1 = P.mode == 3 ? 16 : 8, S2 = P.mode == 3 ? 16 : 8;
        auto W = [&](int m, int period) { return std::pair<double, double>(std::cos(2.0 * PI_D * m / period), -std::sin(2.0 * PI_D * m / period)); };
        for (int k = 1; k < NK1; k++) for (int l = 0; l < LW; l++) { auto w = W(l * k, Mc); blob.push_back(w.first); blob.push_back(w.second); }
        P.o_tw2 = (int)blob.size();
        for (int k = 1; k < 8; k++) for (int q = 0; q < CW; q++) { auto w = W(S2 * q * k, Mc); blob.push_back(w.first); blob.push_back(w.second); }
        P.o_twN = (int)blob.size();
        for (int k = 0; k < Mc; k++) { auto w = W(k, nfft); blob.push_back(w.first); blob.push_back(w.second); }
        P.o_win = (int)blob.size();
        for (int j = 0; j < P.nw; j++) blob.push_back(t.window[(size_t)j]);
        if (blob.size() & 1) blob.push_back(0.0);
        P.o_winR = (int)blob.size();
        for (int k = 0; k <= P.bix; k++) blob.push_back(t.windowR[(size_t)k]);
        if (blob.size() & 1) blob.push_back(0.0);
        P.blob_f64 = (int)blob.size();
    }
}

// ---------------------------------------------------------------------------
// the k_pitch_frames launch
// ---------------------------------------------------------------------------
// k_pitch_frames<WPB, MODE, TABS>: the six instantiations the library holds (pce_pitch.hip maps these to the kernel symbols)
enum PitchFramesKernel { PF_W4_M1, PF_W4_M2_TABS, PF_W4_M3, PF_W4_M0, PF_W2_M0, PF_W1_M0 };
struct PitchFramesLaunch {
    PitchFramesKernel kernel;
    int wpb;            // wavefronts per workgroup
    size_t lds;         // dynamic LDS bytes
    int64_t grid;       // workgroups
};
inline int64_t pitch_frames_grid(int64_t n_work) { return (n_work + 7) & ~(int64_t)7; }   // multiple of 8 so the XCD remap is a bijection; extra blocks exit
inline PitchFramesLaunch pitch_frames_launch(const PiParams &P, int64_t n_work)
{
    PitchFramesLaunch l;
    l.grid = pitch_frames_grid(n_work);
    // long windows (44.1 kHz at a 75 Hz floor: 72 KB per wavefront) run fewer wavefronts per workgroup
    int wpb = PI_WPB;
    while (wpb > 1 && pitch_stockham_wave_bytes(P.zlen) * (size_t)wpb + sizeof(int16_t) * (size_t)P.pcm_span > PI_LDS_LIMIT) wpb >>= 1;
    if (P.mode != 0) wpb = PI_WPB;
    l.wpb = wpb;
    l.lds = P.mode != 0 ? sizeof(double) * ((size_t)reg_wave_f64(P.mode) * PI_WPB + (P.tabs ? (size_t)P.blob_f64 : 0)) + sizeof(int16_t) * (size_t)P.pcm_span
                        : pitch_stockham_wave_bytes(P.zlen) * (size_t)wpb + sizeof(int16_t) * (size_t)P.pcm_span;
    // mode 2 alone has P.tabs
    l.kernel = P.mode == 1 ? PF_W4_M1 : P.mode == 2 ? PF_W4_M2_TABS : P.mode == 3 ? PF_W4_M3 : wpb == 4 ? PF_W4_M0 : wpb == 2 ? PF_W2_M0 : PF_W1_M0;
    return l;
}

// ---------------------------------------------------------------------------
// slice table, work list (one workgroup per P.fpb frames of a slice), frame -> slice table
// ---------------------------------------------------------------------------
struct PitchWork {
    std::vector<PiSlice> slices;        // [max(n, 1)]
    std::vector<PiWork> work;
    std::vector<int> frame_slice;       // [total + 1]
    int np2 = 1;                        // the in-LDS median sort's size; longer slices (a recording of more than 82 s at floor 150) go to k_pitch_median_long
    bool long_slices = false;
    int32_t too_many = -1;              // the first slice with more than INT32_MAX frames (the lists stop there), else -1
};
// clip_off: [n_clips + 1] samples before each clip; frame_off / status / t1: pitch_plan_slices'
inline void pitch_work_make(const pce_slice *slices, int32_t n, const std::vector<int64_t> &clip_off, const std::vector<int64_t> &frame_off,
                            const std::vector<int32_t> &status, const std::vector<double> &t1, int fpb, PitchWork &w)
{
    w.slices.assign((size_t)(n > 0 ? n : 1), PiSlice());
    w.work.clear(); w.frame_slice.clear(); w.too_many = -1;
    int64_t max_frames = 0;
    for (int32_t i = 0; i < n; i++) {
        const pce_slice &s = slices[i];
        PiSlice &h = w.slices[(size_t)i];
        h.begin = s.begin; h.clip_off = clip_off[(size_t)s.clip]; h.clip_len = clip_off[(size_t)s.clip + 1] - clip_off[(size_t)s.clip];
        h.nx = s.end - s.begin; h.frame_off = frame_off[(size_t)i]; h.x1 = s.x1; h.t1 = t1[(size_t)i];
        const int64_t nf = frame_off[(size_t)i + 1] - frame_off[(size_t)i];
        if (nf > INT32_MAX) { w.too_many = i; return; }
        h.n_frames = (int32_t)nf; h.status = status[(size_t)i];
        if (nf > max_frames) max_frames = nf;
        for (int64_t f = 0; f < nf; f += fpb) w.work.push_back({i, (int32_t)f});
    }
    int np2 = 1; while (np2 < max_frames && np2 < PI_MEDIAN_LDS) np2 <<= 1;
    w.np2 = np2;
    w.long_slices = max_frames > PI_MEDIAN_LDS;
    const int64_t total = frame_off[(size_t)n];
    w.frame_slice.assign((size_t)total + 1, 0);
    for (int32_t i = 0; i < n; i++)
        for (int64_t f = frame_off[(size_t)i]; f < frame_off[(size_t)i + 1]; f++) w.frame_slice[(size_t)f] = i;
}

// ---------------------------------------------------------------------------
// bytes of every device buffer the launches write, and the capacities of the two kinds of list
// ---------------------------------------------------------------------------
struct PitchSizes {
    unsigned int list_cap;      // RefineItems one of the RF_LISTS lists holds: every frame of its work items with a full set of candidates
    unsigned int run_cap;       // PathRuns one of the RUN_LISTS lists holds
    size_t item_count_bytes, run_count_bytes;       // the counters in front of the items / runs
    size_t cand, gpeak, psi, f0, strength, summary, runs, dl, rr, items;
};
inline PitchSizes pitch_sizes(const PiParams &P, int64_t total /* frames */, int64_t n_work, size_t n_slice_rows)
{
    PitchSizes z;
    z.list_cap = (unsigned int)((pitch_frames_grid(n_work) + RF_LISTS - 1) / RF_LISTS * P.fpb * (PI_MAXC - 1));
    z.run_cap = (unsigned int)(total / RUN_LISTS + 64);
    z.item_count_bytes = sizeof(unsigned int) * RF_LISTS * RF_CSTRIDE;
    z.run_count_bytes = sizeof(unsigned int) * RUN_LISTS * RF_CSTRIDE;
    z.cand = sizeof(double) * 32 * (size_t)(total + 1);
    z.gpeak = (sizeof(int) + sizeof(double)) * (size_t)(total + 1);   // ncand + intensity
    z.psi = (size_t)PI_MAXC * (size_t)(total + 1) + 16;
    z.f0 = sizeof(double) * (size_t)(total + 1);
    z.strength = sizeof(double) * (size_t)(total + 1);
    z.summary = sizeof(PiSummaryDev) * n_slice_rows;
    z.runs = z.run_count_bytes + sizeof(PathRun) * (size_t)RUN_LISTS * (size_t)(total / RUN_LISTS + 64);
    z.dl = sizeof(double) * 2 * PI_MAXC * (size_t)(total + 1);
    z.rr = sizeof(double) * (size_t)P.rr_half * (size_t)(total + 1);
    // room for the lists at the largest P.fpb (2 PI_FPB) and one more round of lists than n_work + 8 items need: >= RF_LISTS * list_cap
    z.items = sizeof(RefineItem) * (size_t)(PI_MAXC - 1) * (size_t)(2 * PI_FPB) * (size_t)((n_work + 8 + RF_LISTS - 1) / RF_LISTS * RF_LISTS + RF_LISTS)
              + z.item_count_bytes;
    return z;
}
