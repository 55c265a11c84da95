// pce_pitch_path.inc -- Pitch_pathFinder (k_pitch_delta, then k_pitch_path over the runs it lists) and the per-slice voiced summaries
// (k_pitch_median, k_pitch_median_long).  Included by pce_pitch.hip after pce_pitch_fft.inc (wave_sync).

// ---------------------------------------------------------------------------
// Pitch_pathFinder: an elementwise pre-pass, then one wavefront per run of multi-candidate frames
// ---------------------------------------------------------------------------
constexpr int BT_TILE = 256;              // frames per back-tracking tile
constexpr double PATH_VOICELESS = 1e300;

// Elementwise pre-pass of Pitch_pathFinder over every (frame, candidate):
//   dl = {local delta (the finder's first loop), log2 f or PATH_VOICELESS}
// plus the bookkeeping that makes the Viterbi parallel: a frame with a single candidate (the
// voiceless one) is a *cut*: every path passes through it, and the additive constant it
// carries cannot change any later arg-max.  So the recurrence only has to run over maximal
// runs of multi-candidate frames, all runs independently.  Cut frames get their result
// (f0 = 0) here; run starts are appended to RUN_LISTS lists.
__global__ __launch_bounds__(256) void k_pitch_delta(PiParams P, const PiSlice *__restrict__ slices, const int *__restrict__ frame_slice,
                                                    const double *__restrict__ cand, const int *__restrict__ ncand,
                                                    const double *__restrict__ intensity, long long n_frames,
                                                    double2 *__restrict__ dl /* [frames][16] */, double *__restrict__ f0,
                                                    double *__restrict__ strength, PathRun *__restrict__ runs,
                                                    unsigned int *__restrict__ run_count, unsigned int run_cap)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_frames * PI_MAXC) return;
    const long long gi = e >> 4; const int jc = (int)(e & 15);
    const int n_here = ncand[gi];
    const bool real = jc >= 1 && jc < n_here;             // slot 0 is the voiceless candidate; slots >= n do not exist
    const double f = real ? cand[gi * 32 + jc] : 0.0, st = real ? cand[gi * 32 + 16 + jc] : 0.0;
    const double inten = intensity[gi];
    double uv = P.silence_thr <= 0.0 ? 0.0 : 2.0 - inten / (P.silence_thr / (1.0 + P.voicing_thr));
    uv = P.voicing_thr + (uv > 0.0 ? uv : 0.0);
    const bool voiceless_local = f == 0.0 || f > P.ceiling;
    const bool voiceless_trans = f <= 0.0 || f >= P.ceiling;
    const double delta = voiceless_local ? uv : st - P.octave_cost * (log(P.ceiling / f) * LOG2E_D);
    if (jc < max(n_here, 1)) dl[e] = make_double2(delta, voiceless_trans ? PATH_VOICELESS : log(f) * LOG2E_D);
    if (jc == 0) {
        const int n = n_here;
        if (n <= 1) { f0[gi] = 0.0; strength[gi] = 0.0; }
        else {
            const int sl = frame_slice[gi];
            const long long li = gi - slices[sl].frame_off;
            if (li == 0 || ncand[gi - 1] <= 1) {
                const unsigned int list = (unsigned int)(gi >> 2) & (RUN_LISTS - 1);
                const unsigned int pos = atomicAdd(run_count + list * RF_CSTRIDE, 1u);
                runs[(size_t)list * run_cap + pos] = PathRun{gi, slices[sl].frame_off + slices[sl].n_frames, li > 0 ? 1 : 0, 0};
            }
        }
    }
}

// Viterbi over one run of multi-candidate frames per wavefront.  Lane ic (0..15) owns
// candidate ic of the current frame; the previous frame's running delta and log2-frequency
// stay in those lanes' registers and are broadcast with v_readlane (the loop over previous
// candidates is wave-uniform), so the recurrence touches neither a barrier nor global memory.
// Runs are short (speech: tens of frames, a few hundred at most), so everything around the
// recurrence is sized for that: operands arrive in 16-frame chunks (one 16-byte load per lane
// and four frames per instruction, the next chunk in flight while this one is consumed), the
// back-pointers stay in LDS for runs up to PT_CAP frames, and the workgroup is the wavefront
// (no __syncthreads).  Longer runs back-track through global memory in tiles.
constexpr int PT_CHUNK = 16;
constexpr int PT_CAP = 1024;
__global__ __launch_bounds__(64) void k_pitch_path(
    PiParams P, const double *__restrict__ cand, const int *__restrict__ ncand,
    const double2 *__restrict__ dl, const PathRun *__restrict__ runs, const unsigned int *__restrict__ run_count, unsigned int run_cap,
    unsigned char *__restrict__ psi /* [frames][16] */, double *__restrict__ f0, double *__restrict__ strength)
{
    __shared__ double2 t_dl[2][PT_CHUNK][PI_MAXC];
    __shared__ int t_n[2][PT_CHUNK];
    __shared__ __attribute__((aligned(16))) unsigned char t_psi[PT_CAP][PI_MAXC];
    __shared__ unsigned char t_place[PT_CAP];
    static_assert(BT_TILE <= PT_CAP, "the global back-tracking tiles reuse t_psi");
    const int lane = threadIdx.x;
    const int ic = lane & 15;
    const double timeStepCorrection = 0.01 / P.dt;
    const double ojc = P.oj_cost * timeStepCorrection, vuc = P.vuv_cost * timeStepCorrection;
    const unsigned int list = blockIdx.x & (RUN_LISTS - 1);
    const unsigned int count = run_count[list * RF_CSTRIDE];
    for (unsigned int r = blockIdx.x / RUN_LISTS; r < count; r += gridDim.x / RUN_LISTS) {
        const PathRun run = runs[(size_t)list * run_cap + r];
        const long long gs = run.frame, gend = run.gend;
        double pd = 0.0, plf = PATH_VOICELESS;           // previous frame, candidate `ic`
        int pn = 0;
        if (run.has_prev) { pd = dl[(gs - 1) * PI_MAXC].x; pn = 1; }   // the cut frame before the run: one voiceless candidate
        double2 rg[4]; int rn = 0;                        // chunk in flight
        auto fetch = [&](long long g0) {
            const int tn = (int)min((long long)PT_CHUNK, gend - g0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int e = lane + 64 * q;
                rg[q] = (e >> 4) < tn ? dl[g0 * PI_MAXC + e] : make_double2(0.0, 0.0);
            }
            rn = lane < tn ? ncand[g0 + lane] : 0;        // 0 candidates past the slice end: the run stops there
        };
        auto stage = [&](int b) {
#pragma unroll
            for (int q = 0; q < 4; q++) (&t_dl[b][0][0])[lane + 64 * q] = rg[q];
            if (lane < PT_CHUNK) t_n[b][lane] = rn;
        };
        wave_sync();                                      // the previous run's LDS readers are done
        fetch(gs);
        stage(0);
        long long ge = gs;                                // one past the last frame of the run
        int buf = 0;
        bool open = true;
        while (open) {
            const bool more = ge + PT_CHUNK < gend;
            if (more) fetch(ge + PT_CHUNK);
            wave_sync();
            int fr = 0;
            int n2 = t_n[buf][0];
            double2 cur = t_dl[buf][0][ic];
            for (; fr < PT_CHUNK; fr++) {
                if (n2 <= 1) { open = false; break; }
                const int nx = fr + 1 < PT_CHUNK ? fr + 1 : fr;
                const int n2n = t_n[buf][nx];                 // next frame's operands: off the recurrence's critical path
                const double2 nxt = t_dl[buf][nx][ic];
                const double d2 = cur.x, lf2 = cur.y;
                double best = d2; int place = 0;
                if (pn > 0) {
                    best = -1e30;
                    const bool cur_vl = lf2 > 1e299;
                    for (int ic1 = 0; ic1 < pn; ic1++) {
                        const double lf1 = readlane_f64(plf, ic1), d1 = readlane_f64(pd, ic1);
                        const bool pv = lf1 > 1e299;
                        const double tc = (cur_vl != pv) ? vuc : (cur_vl ? 0.0 : ojc * fabs(lf1 - lf2));
                        const double value = d1 - tc + d2;
                        const bool better = value > best;
                        best = better ? value : best; place = better ? ic1 : place;
                    }
                }
                pd = best; plf = lf2; pn = n2;
                const long long idx = ge + fr - gs;
                if (lane < PI_MAXC) {
                    psi[(ge + fr) * PI_MAXC + ic] = (unsigned char)place;
                    if (idx < PT_CAP) t_psi[idx][ic] = (unsigned char)place;
                }
                cur = nxt; n2 = n2n;
            }
            ge += fr;
            if (open) {
                if (more) { stage(buf ^ 1); buf ^= 1; }
                else open = false;
            }
        }
        // choose the end of the path inside the run
        int place = 0;
        {
            double maximum = -1e30;
            const bool cut_follows = ge < gend;          // frame `ge` is a cut frame (single voiceless candidate)
            const double dn = cut_follows ? dl[ge * PI_MAXC].x : 0.0;
            for (int jc = 0; jc < pn; jc++) {
                const double v = readlane_f64(pd, jc), lf = readlane_f64(plf, jc);
                const double value = cut_follows ? (v - ((lf > 1e299) ? 0.0 : vuc) + dn) : v;
                if (jc == 0 || value > maximum) { place = jc; maximum = value; }
            }
        }
        const long long L = ge - gs;
        wave_sync();
        if (L <= PT_CAP) {
            // back-track in LDS (one lane walks the chain), then every lane emits frames
            if (lane == 0) {
                int pl = place;
                for (int i = (int)L - 1; i >= 0; i--) { t_place[i] = (unsigned char)pl; pl = t_psi[i][pl]; }
            }
            wave_sync();
            for (int e = lane; e < (int)L; e += 64) {
                const long long gi = gs + e;
                const int pl = t_place[e];
                f0[gi] = pl ? cand[gi * 32 + pl] : 0.0;
                strength[gi] = pl ? cand[gi * 32 + 16 + pl] : 0.0;
            }
        } else {
            // long run: back-track through the global back-pointers in tiles, last tile first
            __threadfence();
            for (long long hi = ge; hi > gs;) {
                const long long lo = max(gs, hi - BT_TILE);
                const int cnt = (int)(hi - lo);
                for (int e = lane; e < cnt; e += 64)
                    *reinterpret_cast<uint4 *>(&t_psi[e][0]) = *reinterpret_cast<const uint4 *>(psi + (lo + e) * PI_MAXC);
                wave_sync();
                if (lane == 0) {
                    int pl = place;
                    for (int i = cnt - 1; i >= 0; i--) { t_place[i] = (unsigned char)pl; pl = t_psi[i][pl]; }
                    place = pl;
                }
                place = __shfl(place, 0, 64);
                wave_sync();
                for (int e = lane; e < cnt; e += 64) {
                    const long long gi = lo + e;
                    const int pl = t_place[e];
                    f0[gi] = pl ? cand[gi * 32 + pl] : 0.0;
                    strength[gi] = pl ? cand[gi * 32 + 16 + pl] : 0.0;
                }
                wave_sync();
                hi = lo;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// voiced median (np.median) and mean log (-> geometric mean): one workgroup per slice
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pitch_median(const PiSlice *__restrict__ slices, const double *__restrict__ f0,
                                                     int npow2, PiSummaryDev *__restrict__ out)
{
    extern __shared__ double sbuf[];
    __shared__ int s_cnt;
    __shared__ double s_red[4];
    const PiSlice s = slices[blockIdx.x];
    const int tid = threadIdx.x;
    if (s.status != PCE_SLICE_OK || s.n_frames <= 0) {
        if (tid == 0) { out[blockIdx.x].n_voiced = 0; out[blockIdx.x].median = 0.0; out[blockIdx.x].mean_log = 0.0; }
        return;
    }
    if (s.n_frames > npow2) return;                       // longer than the LDS sort holds: k_pitch_median_long's
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const double *f = f0 + s.frame_off;
    double lsum = 0.0;
    for (int i = tid; i < s.n_frames; i += 256) {
        const double v = f[i];
        if (v > 0.0) { const int k = atomicAdd(&s_cnt, 1); sbuf[k] = v; lsum += log(v); }
    }
    __syncthreads();
    const int nv = s_cnt;
    int m = 1; while (m < nv) m <<= 1;
    if (m > npow2) m = npow2;
    for (int i = nv + tid; i < m; i += 256) sbuf[i] = __builtin_huge_val();
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < m; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const double a = sbuf[i], b = sbuf[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { sbuf[i] = b; sbuf[ixj] = a; }
                }
            }
            __syncthreads();
        }
    lsum = wave_xor_sum(lsum);
    if ((tid & 63) == 0) s_red[tid >> 6] = lsum;
    __syncthreads();
    if (tid == 0) {
        PiSummaryDev o;
        o.n_voiced = nv;
        if (nv == 0) { o.median = 0.0; o.mean_log = 0.0; }
        else {
            o.median = (nv & 1) ? sbuf[nv / 2] : (sbuf[nv / 2 - 1] + sbuf[nv / 2]) / 2.0;
            o.mean_log = (((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)nv;
        }
        out[blockIdx.x] = o;
    }
}

// The same summary for a slice of any length (get_median_pitch takes a whole recording, Code/audioPipeline.py:326-335: the reference has no
// limit): the k-th smallest voiced F0 by radix selection on the bit patterns (positive doubles order as their 64-bit integers), eight
// 256-bin passes over the slice's F0 track in global memory per selected rank.  Exact: the median is np.median's (the middle element, or
// the mean of the two middle ones); the log sum adds in the order k_pitch_median adds (per thread by stride 256, then the same tree).
// One workgroup per slice; slices the LDS sort holds return at once.
__global__ __launch_bounds__(256) void k_pitch_median_long(const PiSlice *__restrict__ slices, const double *__restrict__ f0, int lds_limit,
                                                          PiSummaryDev *__restrict__ out)
{
    __shared__ int hist[256];
    __shared__ int s_cnt;
    __shared__ double s_red[4];
    __shared__ unsigned long long s_prefix;
    __shared__ long long s_k;
    const PiSlice s = slices[blockIdx.x];
    const int tid = threadIdx.x;
    if (s.status != PCE_SLICE_OK || s.n_frames <= lds_limit) return;
    const double *f = f0 + s.frame_off;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    double lsum = 0.0; int mine = 0;
    for (int i = tid; i < s.n_frames; i += 256) {
        const double v = f[i];
        if (v > 0.0) { mine++; lsum += log(v); }
    }
    atomicAdd(&s_cnt, mine);
    lsum = wave_xor_sum(lsum);
    if ((tid & 63) == 0) s_red[tid >> 6] = lsum;
    __syncthreads();
    const int nv = s_cnt;
    double sel[2] = {0.0, 0.0};
    const int want = nv == 0 ? 0 : ((nv & 1) ? 1 : 2);
    for (int q = 0; q < want; q++) {
        if (tid == 0) { s_prefix = 0ull; s_k = (nv & 1) ? nv / 2 : nv / 2 - 1 + q; }
        __syncthreads();
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            const unsigned long long prefix = s_prefix;
            for (int i = tid; i < s.n_frames; i += 256) {
                const double v = f[i];
                if (v > 0.0) {
                    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
                    if (shift == 56 || (b >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(int)((b >> shift) & 255ull)], 1);
                }
            }
            __syncthreads();
            if (tid == 0) {
                long long k = s_k; int bin = 0;
                while (bin < 255 && k >= hist[bin]) { k -= hist[bin]; bin++; }
                s_k = k; s_prefix = prefix | ((unsigned long long)bin << shift);
            }
            __syncthreads();
        }
        sel[q] = __longlong_as_double((long long)s_prefix);
        __syncthreads();
    }
    if (tid == 0) {
        PiSummaryDev o;
        o.n_voiced = nv;
        if (nv == 0) { o.median = 0.0; o.mean_log = 0.0; }
        else {
            o.median = (nv & 1) ? sel[0] : (sel[0] + sel[1]) / 2.0;
            o.mean_log = (((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)nv;
        }
        out[blockIdx.x] = o;
    }
}
