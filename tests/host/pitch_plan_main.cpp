// Stand-alone check of csrc/pce_pitch_plan.h (tests/test_pitch_plan_host.py builds it with ASan + UBSan and runs it): which k_pitch_frames
// instantiation a (rate, floor) pair runs and with what launch, the two refusals, the LDS and table-layout invariants over a sweep of rates
// and floors, the bound k_pitch_frames indexes its staged samples against, the tables at spot indices, the work list and the buffer sizes.
// Every vector has exactly the size the plan may read or write.  Exit status 0: every check held.
//   pitch_plan_main                                  run the checks
//   pitch_plan_main plan NX RATE X1 FLOOR CEILING    print pitch_plan_make's status and fields (doubles as hex floats), for the comparison
//                                                    with the oracle's restatement
#include "pce_pitch_plan.h"
#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static pce_pitch_params praat(double floor, double ceiling)
{
    pce_pitch_params p;
    memset(&p, 0, sizeof p);
    p.time_step = 0.0; p.pitch_floor = floor; p.periods_per_window = 3.0; p.max_candidates = 15;
    p.silence_threshold = 0.03; p.voicing_threshold = 0.45; p.octave_cost = 0.01; p.octave_jump_cost = 0.35; p.voiced_unvoiced_cost = 0.14;
    p.pitch_ceiling = ceiling;
    return p;
}

// the plan of a two-second slice that starts at x1, and the kernel parameters made from it
static PitchParamsStatus params_for(int rate, double floor, double ceiling, PitchPlan *pl, PiParams *P, double x1 = 0.0)
{
    const pce_pitch_params p = praat(floor, ceiling);
    const double dx = 1.0 / (double)rate;
    if (x1 == 0.0) x1 = 0.5 * dx;
    CHECK(pitch_plan_make(2 * (int64_t)rate, dx, x1, &p, pl) == PCE_SLICE_OK);
    return pitch_params_make(rate, &p, *pl, false, P);
}

static void instantiations()
{
    struct Case { int rate; double floor; int nfft, mode, fpb, tabs, wpb; PitchFramesKernel kernel; size_t wave_bytes; };
    const Case cases[] = {
        {16000, 150.0, 512, 2, 8, 1, 4, PF_W4_M2_TABS, 0},
        {16000, 75.0, 1024, 1, 4, 0, 4, PF_W4_M1, 0},
        {22050, 150.0, 1024, 1, 4, 0, 4, PF_W4_M1, 0},
        {44100, 150.0, 2048, 3, 4, 0, 4, PF_W4_M3, 0},
        {22050, 75.0, 2048, 3, 4, 0, 4, PF_W4_M3, 0},
        {8000, 150.0, 256, 0, 4, 0, 4, PF_W4_M0, 0},
        {8000, 75.0, 512, 2, 8, 1, 4, PF_W4_M2_TABS, 0},
        {44100, 75.0, 4096, 0, 4, 0, 2, PF_W2_M0, 73792},
        {48000, 50.0, 8192, 0, 4, 0, 1, PF_W1_M0, 147520},
    };
    for (const Case &c : cases) {
        PitchPlan pl; PiParams P;
        CHECK(params_for(c.rate, c.floor, 600.0, &pl, &P) == PITCH_PARAMS_OK);
        const PitchFramesLaunch l = pitch_frames_launch(P, 100);
        CHECK(P.nfft == c.nfft && P.mode == c.mode && P.fpb == c.fpb && P.tabs == c.tabs);
        CHECK(l.kernel == c.kernel && l.wpb == c.wpb && l.grid == 104);
        if (c.wave_bytes) CHECK(pitch_stockham_wave_bytes(P.zlen) == c.wave_bytes);
        if (failures) std::fprintf(stderr, "  (rate %d floor %g: nfft %d mode %d fpb %d tabs %d kernel %d wpb %d)\n", c.rate, c.floor, P.nfft, P.mode, P.fpb,
                                   P.tabs, (int)l.kernel, l.wpb);
    }
    {   // 30 candidates > 16
        PitchPlan pl; PiParams P;
        CHECK(params_for(16000, 20.0, 600.0, &pl, &P) == PITCH_PARAMS_CANDIDATES);
        CHECK(pl.max_candidates == 30);
    }
    {   // 294 976 bytes per wavefront > 160 KB
        PitchPlan pl; PiParams P;
        CHECK(params_for(44100, 20.0, 300.0, &pl, &P) == PITCH_PARAMS_LDS);
        CHECK(pitch_stockham_wave_bytes(P.zlen) == 294976 && P.nw == (int)pl.nsamp_window);
    }
    {   // the refinement mode travels in the parameters
        const pce_pitch_params p = praat(150.0, 600.0);
        PitchPlan pl; PiParams P;
        CHECK(pitch_plan_make(32000, 1.0 / 16000.0, 0.5 / 16000.0, &p, &pl) == PCE_SLICE_OK);
        CHECK(pitch_params_make(16000, &p, pl, true, &P) == PITCH_PARAMS_OK && P.refine_seeded == 0 && P.refine_tol_rel == 3e-8);
        CHECK(pitch_params_make(16000, &p, pl, false, &P) == PITCH_PARAMS_OK && P.refine_seeded == 1);
    }
}

// the window of every frame of a work item lies inside the samples k_pitch_frames stages for it: [lo, lo + pcm_span), with lo and the
// frame's window start ws as the kernel computes them
static void span_holds(const PiParams &P, double t1, double x1, int frame0)
{
    const double tA = t1 + (double)frame0 * P.dt;
    const int64_t lo = (int64_t)std::floor((tA - x1) / P.dx) + 1 - P.hw;
    for (int fi = 0; fi < P.fpb; fi++) {
        const double t = t1 + (double)(frame0 + fi) * P.dt;
        const int64_t ws = (int64_t)std::floor((t - x1) / P.dx) + 1 - P.hw;
        CHECK(ws >= lo && ws + P.nw <= lo + P.pcm_span);
    }
}

static void sweep()
{
    const int rates[] = {8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
    const double floors[] = {50.0, 75.0, 100.0, 150.0, 200.0, 300.0};
    int accepted = 0;
    for (int rate : rates)
        for (double floor : floors) {
            PitchPlan pl; PiParams P;
            if (params_for(rate, floor, 600.0, &pl, &P) != PITCH_PARAMS_OK) continue;
            accepted++;
            PitchTables t;
            pitch_tables_make(pl, P, t);
            const PitchFramesLaunch l = pitch_frames_launch(P, 1000);
            CHECK(l.lds <= PI_LDS_LIMIT && l.grid % 8 == 0 && l.grid >= 1000 && l.grid < 1008);
            CHECK(l.wpb == 1 || l.wpb == 2 || l.wpb == 4);
            CHECK(P.rr_len == 2 * P.bix + 2 && P.rr_half >= P.bix + 1 && P.rr_half % 2 == 0);
            const int Mc = P.nfft / 2;
            CHECK(t.tw.size() == (size_t)(2 * Mc + 1) * 2 && t.window.size() == (size_t)P.nw && t.windowR.size() == (size_t)P.bix + 1);
            if (P.mode == 0) {
                CHECK(t.blob.empty() && P.blob_f64 == 0);
                CHECK(l.lds == pitch_stockham_wave_bytes(P.zlen) * (size_t)l.wpb + 2 * (size_t)P.pcm_span);
                CHECK(P.rr_len <= 2 * P.zlen);                      // r[-bix..bix] fits one of the two complex buffers
            } else {
                const int LW = P.mode == 2 ? 32 : 64, NK1 = P.mode == 3 ? 16 : 8;
                CHECK(Mc == NK1 * LW);
                // r[-bix..bix] fits the frame's exchange region (half of the wavefront's at two frames per wavefront)
                CHECK(P.rr_len <= reg_wave_f64(P.mode) / (P.mode == 2 ? 2 : 1));
                CHECK(P.o_tw2 == 2 * (NK1 - 1) * LW);
                CHECK(P.o_twN == P.o_tw2 + 2 * 7 * LW / 8);
                CHECK(P.o_win == P.o_twN + 2 * Mc);
                CHECK(P.o_winR == P.o_win + ((P.nw + 1) & ~1));
                CHECK(P.blob_f64 == P.o_winR + ((P.bix + 2) & ~1));
                CHECK(P.o_tw2 % 2 == 0 && P.o_twN % 2 == 0 && P.o_win % 2 == 0 && P.o_winR % 2 == 0 && P.blob_f64 % 2 == 0);
                CHECK(t.blob.size() == (size_t)P.blob_f64);
                CHECK(l.lds == 8 * ((size_t)reg_wave_f64(P.mode) * PI_WPB + (P.tabs ? (size_t)P.blob_f64 : 0)) + 2 * (size_t)P.pcm_span);
                // the blob's twN, window and windowR are the plain tables'
                for (int k = 0; k < Mc; k += 37) CHECK(t.blob[(size_t)P.o_twN + 2 * k] == t.tw[2 * (size_t)(Mc + k)] && t.blob[(size_t)P.o_twN + 2 * k + 1] == t.tw[2 * (size_t)(Mc + k) + 1]);
                for (int j = 0; j < P.nw; j += 29) CHECK(t.blob[(size_t)P.o_win + j] == t.window[(size_t)j]);
                for (int k = 0; k <= P.bix; k += 31) CHECK(t.blob[(size_t)P.o_winR + k] == t.windowR[(size_t)k]);
                // tw1[k - 1][l] = W_M^(l k)
                const int k = NK1 - 1, lane = LW - 3;
                CHECK(t.blob[2 * (size_t)((k - 1) * LW + lane)] == std::cos(2.0 * PI_D * (lane * k) / Mc));
                CHECK(t.blob[2 * (size_t)((k - 1) * LW + lane) + 1] == -std::sin(2.0 * PI_D * (lane * k) / Mc));
            }
            CHECK(P.pcm_span % 8 == 0);
            // whole slices that start at sample 0, at a praat_part_frames-style cut (x1 = an odd number of samples and a half) and at a time
            // that is no multiple of dx; the first, middle and last work items
            const pce_pitch_params p = praat(floor, 600.0);
            const double x1s[] = {0.5 * P.dx, 12345.5 * P.dx, 0.123456789, -3.25 * P.dx};
            for (double x1 : x1s) {
                PitchPlan q;
                const int64_t nx = 2 * (int64_t)rate - 7;
                CHECK(pitch_plan_make(nx, P.dx, x1, &p, &q) == PCE_SLICE_OK);
                const int last = (int)((q.n_frames - 1) / P.fpb) * P.fpb;
                const int f0s[] = {0, P.fpb, last / 2 / P.fpb * P.fpb, last};
                for (int frame0 : f0s) span_holds(P, q.t1, x1, frame0);
            }
        }
    CHECK(accepted >= 40);
}

static void tables()
{
    PitchPlan pl; PiParams P; PitchTables t;
    CHECK(params_for(16000, 75.0, 600.0, &pl, &P) == PITCH_PARAMS_OK);
    pitch_tables_make(pl, P, t);
    const int Mc = P.nfft / 2;
    const int ms[] = {0, 1, Mc / 4, Mc / 2 + 3, Mc - 1};
    for (int m : ms) {
        CHECK(t.tw[2 * (size_t)m] == std::cos(2.0 * PI_D * m / Mc) && t.tw[2 * (size_t)m + 1] == -std::sin(2.0 * PI_D * m / Mc));
        CHECK(std::fabs(t.tw[2 * (size_t)m] * t.tw[2 * (size_t)m] + t.tw[2 * (size_t)m + 1] * t.tw[2 * (size_t)m + 1] - 1.0) < 1e-15);
    }
    const int ks[] = {0, 1, Mc / 2, Mc};
    for (int k : ks)
        CHECK(t.tw[2 * (size_t)(Mc + k)] == std::cos(2.0 * PI_D * k / P.nfft) && t.tw[2 * (size_t)(Mc + k) + 1] == -std::sin(2.0 * PI_D * k / P.nfft));
    CHECK(t.tw[0] == 1.0 && t.tw[1] == 0.0 && std::fabs(t.tw[2 * (size_t)(Mc + Mc)] + 1.0) < 1e-15);       // W^0 = 1, W_N^(N/2) = -1
    // the Hanning window is symmetric and positive, its normalised autocorrelation starts at 1 and never exceeds it
    for (int j = 0; j < P.nw; j++) {
        CHECK(std::fabs(t.window[(size_t)j] - t.window[(size_t)(P.nw - 1 - j)]) < 1e-15);
        CHECK(t.window[(size_t)j] > 0.0 && t.window[(size_t)j] <= 1.0);
    }
    CHECK(t.windowR[0] == 1.0);
    for (int k = 0; k <= P.bix; k++) CHECK(std::fabs(t.windowR[(size_t)k]) <= 1.0);
    for (int k = 1; k <= P.bix; k++) CHECK(t.windowR[(size_t)k] < t.windowR[(size_t)(k - 1)]);
}

static pce_slice slice(int32_t clip, int64_t begin, int64_t end, double x1)
{
    pce_slice s; memset(&s, 0, sizeof s);
    s.clip = clip; s.begin = begin; s.end = end; s.x1 = x1;
    return s;
}

static void work_lists()
{
    const pce_pitch_params p = praat(150.0, 600.0);
    const int rate = 16000;
    const double dx = 1.0 / rate;
    std::vector<int64_t> fo; std::vector<int32_t> st; std::vector<double> t1;
    PitchPlan common; int why = 0;
    {   // three clips; slices: analysable, too short, empty, analysable and shorter
        const std::vector<int64_t> clip_off{0, 16000, 16100, 40000};
        const std::vector<pce_slice> sl{slice(0, 0, 16000, 0.5 * dx), slice(1, 0, 100, 0.5 * dx), slice(2, 50, 50, 0.0), slice(2, 1000, 9000, 1000.5 * dx)};
        CHECK(pitch_plan_slices(rate, 3, &p, sl.data(), 4, fo, st, t1, &common, &why) == -1);
        CHECK(fo.size() == 5 && st == (std::vector<int32_t>{PCE_SLICE_OK, PCE_SLICE_TOO_SHORT, PCE_SLICE_EMPTY, PCE_SLICE_OK}));
        CHECK(fo[0] == 0 && fo[1] == common.n_frames && fo[2] == fo[1] && fo[3] == fo[1] && fo[4] > fo[3]);
        PitchPlan pl; PiParams P;
        CHECK(params_for(rate, 150.0, 600.0, &pl, &P) == PITCH_PARAMS_OK && P.fpb == 8);
        PitchWork w;
        pitch_work_make(sl.data(), 4, clip_off, fo, st, t1, P.fpb, w);
        CHECK(w.too_many == -1 && w.slices.size() == 4 && w.frame_slice.size() == (size_t)fo[4] + 1);
        const int64_t n0 = fo[1], n3 = fo[4] - fo[3];
        CHECK(w.work.size() == (size_t)((n0 + 7) / 8 + (n3 + 7) / 8));
        size_t at = 0;
        for (int64_t f = 0; f < n0; f += 8, at++) CHECK(w.work[at].slice == 0 && w.work[at].frame0 == f);
        for (int64_t f = 0; f < n3; f += 8, at++) CHECK(w.work[at].slice == 3 && w.work[at].frame0 == f);
        CHECK(at == w.work.size());
        CHECK(w.slices[1].n_frames == 0 && w.slices[1].status == PCE_SLICE_TOO_SHORT && w.slices[2].status == PCE_SLICE_EMPTY);
        CHECK(w.slices[3].clip_off == 16100 && w.slices[3].clip_len == 23900 && w.slices[3].begin == 1000 && w.slices[3].nx == 8000 &&
              w.slices[3].frame_off == fo[3] && w.slices[3].t1 == t1[3] && w.slices[3].n_frames == (int32_t)n3);
        CHECK(w.frame_slice[0] == 0 && w.frame_slice[(size_t)n0 - 1] == 0 && w.frame_slice[(size_t)n0] == 3 && w.frame_slice[(size_t)fo[4] - 1] == 3);
        int np2 = 1; while (np2 < n0) np2 <<= 1;
        CHECK(w.np2 == np2 && !w.long_slices);
        // a slice that names no clip, a slice that ends before it begins
        const std::vector<pce_slice> bad1{sl[0], slice(3, 0, 10, 0.0)}, bad2{slice(0, 10, 9, 0.0)};
        CHECK(pitch_plan_slices(rate, 3, &p, bad1.data(), 2, fo, st, t1, &common, &why) == 1 && why == 1);
        CHECK(pitch_plan_slices(rate, 3, &p, bad2.data(), 1, fo, st, t1, &common, &why) == 0 && why == 2);
    }
    {   // an empty batch, and a batch of slices that are all too short: no work, one slice row, the zero plan
        const std::vector<int64_t> clip_off{0, 16000};
        CHECK(pitch_plan_slices(rate, 1, &p, nullptr, 0, fo, st, t1, &common, &why) == -1 && fo == std::vector<int64_t>{0} && common.nsamp_window == 0);
        PitchWork w;
        pitch_work_make(nullptr, 0, clip_off, fo, st, t1, 0, w);
        CHECK(w.work.empty() && w.slices.size() == 1 && w.frame_slice.size() == 1 && w.np2 == 1 && !w.long_slices);
        const std::vector<pce_slice> sl{slice(0, 0, 100, 0.0), slice(0, 5, 5, 0.0)};
        CHECK(pitch_plan_slices(rate, 1, &p, sl.data(), 2, fo, st, t1, &common, &why) == -1 && fo == (std::vector<int64_t>{0, 0, 0}));
        CHECK(common.nsamp_window == 0 && common.n_frames == 0 && common.dt == 0.0);
        pitch_work_make(sl.data(), 2, clip_off, fo, st, t1, 0, w);
        CHECK(w.work.empty() && w.slices.size() == 2 && w.slices[0].status == PCE_SLICE_TOO_SHORT && w.slices[1].status == PCE_SLICE_EMPTY && w.np2 == 1);
    }
    {   // the in-LDS median holds 16 384 frames: a slice of exactly that many, and of one more
        const std::vector<int64_t> clip_off{0, 1}; const std::vector<int32_t> ok{PCE_SLICE_OK}; const std::vector<double> tt{0.0};
        const std::vector<pce_slice> sl{slice(0, 0, 1, 0.0)};
        PitchWork w;
        pitch_work_make(sl.data(), 1, clip_off, std::vector<int64_t>{0, 16384}, ok, tt, 8, w);
        CHECK(w.np2 == 16384 && !w.long_slices && w.work.size() == 2048 && w.frame_slice.size() == 16385);
        pitch_work_make(sl.data(), 1, clip_off, std::vector<int64_t>{0, 16385}, ok, tt, 8, w);
        CHECK(w.np2 == 16384 && w.long_slices && w.work.size() == 2049 && w.work.back().frame0 == 16384);
        pitch_work_make(sl.data(), 1, clip_off, std::vector<int64_t>{0, 8193}, ok, tt, 4, w);
        CHECK(w.np2 == 16384 && !w.long_slices && w.work.size() == 2049);
        pitch_work_make(sl.data(), 1, clip_off, std::vector<int64_t>{0, (int64_t)INT32_MAX + 1}, ok, tt, 8, w);
        CHECK(w.too_many == 0 && w.work.empty());
    }
}

static void sizes()
{
    PiParams P; memset(&P, 0, sizeof P);
    P.bix = 159; P.rr_half = 160;
    const int64_t n_works[] = {0, 1, 7, 8, 255, 256, 257};
    const int fpbs[] = {PI_FPB, 2 * PI_FPB};
    for (int fpb : fpbs)
        for (int64_t n_work : n_works) {
            P.fpb = fpb;
            const int64_t total = n_work * fpb;
            const PitchSizes z = pitch_sizes(P, total, n_work, 3);
            const int64_t grid = pitch_frames_grid(n_work);
            // every list holds the candidates of all frames of its share of the workgroups (workgroup b appends to list b mod RF_LISTS)
            CHECK((int64_t)z.list_cap == (grid + RF_LISTS - 1) / RF_LISTS * fpb * (PI_MAXC - 1));
            CHECK(z.items >= z.item_count_bytes + sizeof(RefineItem) * (size_t)RF_LISTS * (size_t)z.list_cap);
            CHECK(z.item_count_bytes == 4u * RF_LISTS * RF_CSTRIDE && z.run_count_bytes == 4u * RUN_LISTS * RF_CSTRIDE);
            // a run starts at most at every second frame; frame g's start goes to list (g / 4) mod RUN_LISTS
            CHECK((int64_t)z.run_cap == total / RUN_LISTS + 64 && z.runs == z.run_count_bytes + sizeof(PathRun) * (size_t)RUN_LISTS * z.run_cap);
            CHECK(z.cand == 8u * 32 * (size_t)(total + 1) && z.dl == 16u * PI_MAXC * (size_t)(total + 1) && z.psi >= (size_t)PI_MAXC * (size_t)total);
            CHECK(z.gpeak == 12u * (size_t)(total + 1) && z.f0 == 8u * (size_t)(total + 1) && z.strength == z.f0);
            CHECK(z.rr == 8u * 160 * (size_t)(total + 1) && z.summary == 3 * sizeof(PiSummaryDev));
        }
    static_assert(sizeof(RefineItem) == 16 && sizeof(PathRun) == 24 && sizeof(PiWork) == 8 && sizeof(PiSummaryDev) == 24, "device records");
}

static int print_plan(char **a)
{
    const int64_t nx = std::strtoll(a[0], nullptr, 10);
    const int rate = std::atoi(a[1]);
    const double x1 = std::strtod(a[2], nullptr);
    const pce_pitch_params p = praat(std::strtod(a[3], nullptr), std::strtod(a[4], nullptr));
    PitchPlan pl; memset(&pl, 0, sizeof pl);
    const int st = pitch_plan_make(nx, 1.0 / (double)rate, x1, &p, &pl);
    std::printf("status %d\n", st);
    if (st != PCE_SLICE_OK) return 0;
    PiParams P;
    const PitchParamsStatus ps = pitch_params_make(rate, &p, pl, false, &P);
    std::printf("dt %a\nt1 %a\nceiling %a\ndt_window %a\n", pl.dt, pl.t1, pl.ceiling, pl.dt_window);
    std::printf("n_frames %lld\nnsamp_period %lld\nhalfnsamp_period %lld\nnsamp_window %lld\nhalfnsamp_window %lld\n", (long long)pl.n_frames,
                (long long)pl.nsamp_period, (long long)pl.halfnsamp_period, (long long)pl.nsamp_window, (long long)pl.halfnsamp_window);
    std::printf("maximum_lag %lld\nbrent_ixmax %lld\nmax_candidates %lld\n", (long long)pl.maximum_lag, (long long)pl.brent_ixmax, (long long)pl.max_candidates);
    if (ps != PITCH_PARAMS_CANDIDATES) std::printf("nsamp_fft %d\n", P.nfft);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && std::strcmp(argv[1], "plan") == 0) return print_plan(argv + 2);
    if (argc != 1) { std::fprintf(stderr, "usage: %s [plan NX RATE X1 FLOOR CEILING]\n", argv[0]); return 2; }
    instantiations();
    sweep();
    tables();
    work_lists();
    sizes();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
