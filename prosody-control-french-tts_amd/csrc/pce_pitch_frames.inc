// pce_pitch_frames.inc -- k_pitch_frames: windowed frame -> autocorrelation by FFT -> local maxima -> candidate lags handed to k_pitch_refine,
// and the wave-wide sinc interpolation its rare path needs.  Included by pce_pitch.hip after pce_pitch_fft.inc.

// Praat NUM_interpolate_sinc with its terms spread over the wave.  y is the LDS image of
// r[-bix..bix] (0-based storage of Praat's 1-based y[1..nx]); every lane passes the same x
// and receives the same result.
__device__ double sinc_wave(const double *y, int nx, double x, int maxDepth, int lane)
{
    const int midleft = (int)floor(x), midright = midleft + 1;
    if (x > (double)nx) return y[nx - 1];
    if (x < 1.0) return y[0];
    if (x == (double)midleft) return y[midleft - 1];
    if (maxDepth > midright - 1) maxDepth = midright - 1;
    if (maxDepth > nx - midleft) maxDepth = nx - midleft;
    if (maxDepth <= 0) return y[(int)floor(x + 0.5) - 1];
    if (maxDepth == 1) return y[midleft - 1] + (x - (double)midleft) * (y[midright - 1] - y[midleft - 1]);
    if (maxDepth == 2) {
        const double yl = y[midleft - 1], yr = y[midright - 1];
        const double dyl = 0.5 * (yr - y[midleft - 2]), dyr = 0.5 * (y[midright] - yl);
        const double fil = x - (double)midleft, fir = (double)midright - x;
        return yl * fir + yr * fil - fil * fir * (0.5 * (dyr - dyl) + (fil - 0.5) * (dyl + dyr - 2.0 * (yr - yl)));
    }
    const int left = midright - maxDepth, right = midleft + maxDepth;
    const double a_l = PI_D * (x - (double)midleft), a_r = PI_D * ((double)midright - x);
    const double hs_l = 0.5 * sin(a_l), hs_r = 0.5 * sin(a_r);
    const double den_l = x - (double)left + 1.0, den_r = (double)right - x + 1.0;
    const double aa_l = a_l / den_l, daa_l = PI_D / den_l;
    const double aa_r = a_r / den_r, daa_r = PI_D / den_r;
    double acc = 0.0;
    for (int t = lane; t < 2 * maxDepth; t += 64) {
        const bool is_left = t < maxDepth;
        const int k = is_left ? t : t - maxDepth;
        const double kd = (double)k;
        const double a = (is_left ? a_l : a_r) + kd * PI_D;
        const double aa = (is_left ? aa_l : aa_r) + kd * (is_left ? daa_l : daa_r);
        double hs = is_left ? hs_l : hs_r;
        if (k & 1) hs = -hs;
        const int ix = is_left ? midleft - k : midright + k;          // 1-based
        const double d = hs / a * (1.0 + cos(aa));
        acc += y[ix - 1] * d;
    }
    return wave_xor_sum(acc);
}

// MODE 0: any N, one frame per wavefront, Stockham passes between two LDS buffers.
// MODE 1: N = 1024, one frame per wavefront, register-resident transform.
// MODE 2: N = 512 (16 kHz at the reference's 150 Hz floor, Code/audioPipeline.py:329), TWO frames per
//         wavefront (one per 32-lane half), register-resident transform.
// MODE 3: N = 2048 (44.1 kHz at that floor), one frame per wavefront, 16 points per lane.
template <int WPB, int MODE, bool TABS>
__global__ __launch_bounds__(64 * WPB) void k_pitch_frames(
    const int16_t *__restrict__ pcm, const PiSlice *__restrict__ slices, const PiWork *__restrict__ work, int n_work,
    PiParams P, const double *__restrict__ window, const double *__restrict__ windowR,
    const double2 *__restrict__ twM /* exp(-2 pi i m / M), m < M */, const double2 *__restrict__ twN /* exp(-2 pi i k / N), k <= M */,
    const long long *acc_sum, const int *acc_hi, const int *acc_lo, size_t acc_stride,
    double *__restrict__ cand /* [frames][32]: 16 freq, 16 strength */, int *__restrict__ ncand, double *__restrict__ intensity,
    double *__restrict__ rr_out /* [frames][rr_half]: r[0..bix] */, RefineItem *__restrict__ items, unsigned int *__restrict__ item_count,
    unsigned int list_cap, const double *__restrict__ blob /* register paths: lane-ordered twiddles, twN, window, windowR */)
{
    // the LUFS chain runs beside this kernel on a side stream (few waves, long dependent fp64 chains): with this kernel's
    // waves at a higher issue priority it only takes the slots they leave (2.94 -> 2.88 ms per step; raising the
    // priority of the path / median kernels beside the STFT pass changed nothing)
    __builtin_amdgcn_s_setprio(2);
    constexpr int LW = MODE == 2 ? 32 : 64;              // lanes per frame
    constexpr int FPW = 64 / LW;                         // frames per wavefront
    constexpr int FPB = MODE == 2 ? 2 * PI_FPB : PI_FPB; // frames per work item (host: P.fpb)
    constexpr int MR = (MODE == 3 ? 16 : 8) * LW;        // M on the register paths
    constexpr int R = MODE == 3 ? 16 : 8;                // complex points per lane on the register paths
    constexpr int RW = reg_wave_f64(MODE);               // doubles of LDS per wavefront there
    constexpr int REG_C = RW / 2 / FPW;                  // complex slots per frame on the register paths
    extern __shared__ double lds[];
    // XCD-aware remap: consecutive work items (overlapping windows of one slice) go to one XCD's L2
    const int nb = (int)gridDim.x;
    int bid = (int)blockIdx.x;
    if ((nb & 7) == 0) bid = (bid & 7) * (nb >> 3) + (bid >> 3);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int hl = lane & (LW - 1), half = lane / LW;    // lane within the frame's group; the group
    const int M = P.nfft >> 1;
    if (bid >= n_work) return;
    const PiWork wk = work[bid];
    const PiSlice s = slices[wk.slice];
    double2 *wave_base = reinterpret_cast<double2 *>(lds) + (MODE == 0 ? (size_t)wv * (size_t)(2 * P.zlen) : (size_t)wv * (reg_wave_f64(MODE) / 2));
    double2 *bufA = MODE == 0 ? wave_base : wave_base + half * REG_C;
    double2 *bufB = bufA + P.zlen;                      // (MODE 0 only)
    double *xr = reinterpret_cast<double *>(bufA);      // MODE 0: real view of bufA: x[j] at xr[2 ZP(j>>1) + (j&1)]
    // register paths: the tables (optionally) and the samples under this work item's frames go to LDS once
    // per workgroup -- per-lane 2-byte and gather loads were the bottleneck (vector-memory issue, not bytes)
    const double2 *tw1 = nullptr, *tw2 = nullptr, *twR = nullptr;
    const double *win = nullptr, *winR = nullptr;
    const int16_t *spcm = nullptr;
    int64_t lo = 0;
    if constexpr (MODE != 0) {
        double *tab = lds + WPB * RW;
        if constexpr (TABS) {
            for (int i = (int)threadIdx.x; i < (P.blob_f64 >> 1); i += 64 * WPB)
                reinterpret_cast<double2 *>(tab)[i] = reinterpret_cast<const double2 *>(blob)[i];
            tw1 = reinterpret_cast<const double2 *>(tab); tw2 = reinterpret_cast<const double2 *>(tab + P.o_tw2);
            twR = reinterpret_cast<const double2 *>(tab + P.o_twN); win = tab + P.o_win; winR = tab + P.o_winR;
        } else {
            tw1 = reinterpret_cast<const double2 *>(blob); tw2 = reinterpret_cast<const double2 *>(blob + P.o_tw2);
            twR = reinterpret_cast<const double2 *>(blob + P.o_twN); win = blob + P.o_win; winR = blob + P.o_winR;
        }
    }
    {   // every mode: the samples under this work item's frames, staged once per workgroup
        int16_t *sp = MODE != 0 ? reinterpret_cast<int16_t *>(lds + WPB * RW + (TABS ? P.blob_f64 : 0))
                                : reinterpret_cast<int16_t *>(lds + (size_t)WPB * 4 * (size_t)P.zlen);
        const double tA = s.t1 + (double)wk.frame0 * P.dt;
        lo = (int64_t)floor((tA - s.x1) / P.dx) + 1 - P.hw;       // window start of the first frame (slice-relative)
        for (int i = (int)threadIdx.x; i < P.pcm_span; i += 64 * WPB) {
            const int64_t rel = lo + i, cc = s.begin + rel;
            int v = 0;
            if (rel >= 0 && rel < s.nx && cc >= 0 && cc < s.clip_len) v = (int)pcm[s.clip_off + cc];
            sp[i] = (int16_t)v;
        }
        spcm = sp;
        __syncthreads();
    }
    for (int fi = wv * FPW; fi < FPB; fi += WPB * FPW) {
    const int iframe = wk.frame0 + fi + half;           // 0-based
    const bool live = iframe < s.n_frames;
    if (__ballot(live) == 0) break;
    const int64_t fidx = s.frame_off + iframe;
    wave_sync();                                        // the previous frame's LDS reads are done

    // global mean / peak of the slice from the exact integer accumulators
    double globalPeak;
    {
        const char *base = reinterpret_cast<const char *>(acc_sum) + acc_stride * (size_t)wk.slice;
        const long long isum = *reinterpret_cast<const long long *>(base);
        int hi = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(acc_hi) + acc_stride * (size_t)wk.slice);
        int lo = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(acc_lo) + acc_stride * (size_t)wk.slice);
        if (s.begin < 0 || s.begin + s.nx > s.clip_len) { hi = max(hi, 32769); lo = max(lo, 32768); }   // virtual zeros
        const double xmax = hi ? (double)(hi - 32769) / 32768.0 : 0.0;
        const double xmin = lo ? (double)(32768 - lo) / 32768.0 : 0.0;
        const double mean = ((double)isum / 32768.0) / (double)s.nx;
        globalPeak = fmax(fabs(xmax - mean), fabs(xmin - mean));
    }

    // frame position: Sampled_indexToX / Sampled_xToLowIndex
    const double t = s.t1 + (double)iframe * P.dt;
    const int64_t L0 = (int64_t)floor((t - s.x1) / P.dx);        // leftSample - 1 (0-based)
    const int64_t ws = L0 + 1 - P.hw;                             // first sample of the window (slice-relative)
    const int64_t m0 = L0 + 1 - P.nsp, m1 = L0 + P.nsp;           // local-mean range, inclusive

    double2 z[R];                                        // register paths: z[r] = x[2n] + i x[2n+1], n = hl + LW r
    double lpk = 0.0;
    const int pk0 = max(P.hw + 1 - P.hsp, 1), pk1 = min(P.hw + P.hsp, P.nw);   // 1-based inclusive
    if constexpr (MODE != 0) {
        int isum = 0, v[2 * R];
#pragma unroll
        for (int r = 0; r < R; r++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int j = 2 * (hl + LW * r) + h;
                int x = 0;
                if (live && j < P.nw) {
                    const int64_t rel = ws + j;
                    x = (int)spcm[(int)(ws - lo) + j];
                    if (rel >= m0 && rel <= m1) isum += x;
                }
                v[2 * r + h] = x;
            }
        }
        isum = wave_xor_sum<LW>(isum);
        const double localMean = ((double)isum / 32768.0) / (double)(2 * P.nsp);
#pragma unroll
        for (int r = 0; r < R; r++) {
            double f[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int j = 2 * (hl + LW * r) + h;
                f[h] = 0.0;
                if (live && j < P.nw) {
                    f[h] = ((double)v[2 * r + h] / 32768.0 - localMean) * win[j];
                    if (j + 1 >= pk0 && j + 1 <= pk1) lpk = fmax(lpk, fabs(f[h]));
                }
            }
            z[r] = make_double2(f[0], f[1]);
        }
    } else {
    // stage raw samples (exact in fp64) and the integer local sum
    int isum = 0;
    for (int j = lane; j < P.nfft; j += 64) {
        int v = 0;
        if (j < P.nw) {
            const int64_t rel = ws + j;
            v = (int)spcm[(int)(ws - lo) + j];
            if (rel >= m0 && rel <= m1) isum += v;
        }
        xr[2 * ZP(j >> 1) + (j & 1)] = (double)v / 32768.0;
    }
    isum = wave_xor_sum(isum);
    const double localMean = ((double)isum / 32768.0) / (double)(2 * P.nsp);
    for (int j = lane; j < P.nw; j += 64) {
        const int a = 2 * ZP(j >> 1) + (j & 1);
        const double f = (xr[a] - localMean) * window[j];
        xr[a] = f;
        if (j + 1 >= pk0 && j + 1 <= pk1) lpk = fmax(lpk, fabs(f));
    }
    }
    const double localPeak = wave_xor_max<LW>(lpk);
    // (a slice without a peak -- all zeros, or one constant -- has intensity 0 in every frame, as Praat leaves it: not 0 / 0)
    const double inten = globalPeak == 0.0 ? 0.0 : localPeak > globalPeak ? 1.0 : localPeak / globalPeak;
    const bool active = live && localPeak != 0.0;

    double *rr = nullptr;                                // rr[bix + k] = r[k], k in [-bix, bix]
    // candidate registers: group lane q holds candidate q (0 = the voiceless candidate)
    double c_f = 0.0, c_s = 0.0; int c_i = 0; int n = 1;

    if (__ballot(active) != 0) {
        if constexpr (MODE != 0) {
            wave_sync();
            if constexpr (MODE == 1) fft512_reg(z, bufA, tw1, tw2, lane); else if constexpr (MODE == 3) fft1024_reg(z, bufA, tw1, tw2, lane); else fft256_half(z, bufA, tw1, tw2, hl);
            // power spectrum of the real frame, re-tangled for the second transform.  Lane-local form of
            // the pairwise loop of MODE 0: for every own k, with zm = Z[M - k],
            // X[k] = ez + t, X[M - k]* = ez - t, and W[k] = (e - d sin, -d cos) holds for all k in [0, M).
#pragma unroll
            for (int r = 0; r < R; r++) bufA[hl + LW * r] = z[r];
            wave_sync();
#pragma unroll
            for (int r = 0; r < R; r++) {
                const int k = hl + LW * r;
                const double2 zk = z[r], zm = bufA[(MR - k) & (MR - 1)];
                const double2 w = twR[k];                                     // (cos, -sin)
                const double2 ez = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
                const double2 oz = make_double2(0.5 * (zk.y + zm.y), -0.5 * (zk.x - zm.x));
                const double2 t = cmul_f64(oz, w);
                const double xr1 = ez.x + t.x, xi1 = ez.y + t.y, xr2 = ez.x - t.x, xi2 = ez.y - t.y;
                const double pk = fma(xr1, xr1, xi1 * xi1), pm = fma(xr2, xr2, xi2 * xi2);
                const double e = 0.5 * (pk + pm), d = 0.5 * (pk - pm);
                z[r] = make_double2(e - d * (-w.y), -(d * w.x));
            }
            wave_sync();
            if constexpr (MODE == 1) fft512_reg(z, bufA, tw1, tw2, lane); else if constexpr (MODE == 3) fft1024_reg(z, bufA, tw1, tw2, lane); else fft256_half(z, bufA, tw1, tw2, hl);
            // ac[2n] = Re Y[n], ac[2n+1] = -Im Y[n]; r[k] = ac[k] / (ac[0] windowR[k]) into the same region
            // (reciprocal to < 1 ulp and a multiply: the quotient is not correctly rounded, like the transforms before it)
            rr = reinterpret_cast<double *>(bufA);
            const double ac0 = __shfl(z[0].x, lane & ~(LW - 1), 64);
            if (active) {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int k = 2 * (hl + LW * r);
                    if (k >= 1 && k <= P.bix) { const double v = z[r].x * rcp_f64(ac0 * winR[k]); rr[P.bix + k] = v; rr[P.bix - k] = v; }
                    if (k + 1 <= P.bix) { const double v = -z[r].y * rcp_f64(ac0 * winR[k + 1]); rr[P.bix + k + 1] = v; rr[P.bix - k - 1] = v; }
                }
                if (hl == 0) rr[P.bix] = 1.0;
            }
            wave_sync();
        } else {
        wave_sync();
        // forward transform of the packed frame
        double2 *Z = fft_wave(bufA, bufB, M, twM, lane);
        double2 *W = (Z == bufA) ? bufB : bufA;
        // power spectrum of the real frame, re-tangled for the second (inverse) transform
        for (int k = lane; k <= (M >> 1); k += 64) {
            const double2 zk = Z[ZP(k & (M - 1))], zm = Z[ZP((M - k) & (M - 1))];
            const double2 w = twN[k];                                     // (cos, -sin)
            const double2 ez = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y));
            const double2 oz = make_double2(0.5 * (zk.y + zm.y), -0.5 * (zk.x - zm.x));
            const double2 t = cmul_f64(oz, w);
            const double xr1 = ez.x + t.x, xi1 = ez.y + t.y, xr2 = ez.x - t.x, xi2 = ez.y - t.y;
            const double pk = fma(xr1, xr1, xi1 * xi1), pm = fma(xr2, xr2, xi2 * xi2);
            const double e = 0.5 * (pk + pm), d = 0.5 * (pk - pm);
            const double c = w.x, sn = -w.y;
            W[ZP(k & (M - 1))] = make_double2(e - d * sn, -(d * c));
            if (k != 0 && k != M - k) W[ZP(M - k)] = make_double2(e + d * sn, -(d * c));
        }
        wave_sync();
        double2 *Y = fft_wave(W, Z, M, twM, lane);
        rr = reinterpret_cast<double *>((Y == bufA) ? bufB : bufA);       // the free buffer holds r[-bix..bix]
        const double ac0 = Y[0].x;
        for (int k = lane + 1; k <= P.bix; k += 64) {
            const double2 y = Y[ZP(k >> 1)];
            const double ack = (k & 1) ? -y.y : y.x;
            const double v = ack / (ac0 * windowR[k]);
            rr[P.bix + k] = v; rr[P.bix - k] = v;
        }
        if (lane == 0) rr[P.bix] = 1.0;
        wave_sync();
        }

        const int ynx = 2 * P.bix + 1;
        const int lim = min(P.maxlag, P.bix);
        const double half_vt = 0.5 * P.voicing_thr;
        // count the local maxima first: with at most maxc-1 of them (the common case) every
        // maximum becomes a candidate and the first-pass strength is never consulted.
        int total = 0;
        for (int base = 2; base < lim; base += LW) {
            const int i = base + hl;
            bool pred = false;
            if (active && i < lim) {
                const double r0 = rr[P.bix + i], rm = rr[P.bix + i - 1], rp = rr[P.bix + i + 1];
                pred = r0 > half_vt && r0 > rm && r0 >= rp;
            }
            unsigned long long mask = __ballot(pred);
            if (LW == 32) mask = (mask >> (32 * half)) & 0xffffffffull;
            const int here = __popcll(mask);
            if (total + here <= P.maxc - 1) {
                // the lane that owns slot (1 + total + q) takes the lag of the q-th maximum of this round
                const int need = hl - 1 - total;
                if (need >= 0 && need < here) {
                    unsigned long long m = mask;
                    for (int q = 0; q < need; q++) m &= m - 1;
                    c_i = base + __ffsll((long long)m) - 1;
                }
            }
            total += here;
        }
        const bool rare = total > P.maxc - 1;
        if (!rare) n = 1 + total;
        // rare: more maxima than candidate slots -> Praat's replacement rule needs first-pass strengths.
        // The whole wavefront works on one frame at a time here (sinc_wave spreads its terms over 64 lanes).
        const unsigned long long rare_mask = __ballot(rare);
        for (int g = 0; g < FPW; g++) {
            if (!((rare_mask >> (g * LW)) & 1ull)) continue;
            const double *rg = FPW == 1 ? rr : reinterpret_cast<const double *>(wave_base + g * REG_C);
            const bool mine = half == g;
            int ng = 1;
            if (mine) c_i = 0;
            for (int base = 2; base < lim; base += 64) {
                const int i = base + lane;
                bool pred = false;
                if (i < lim) {
                    const double r0 = rg[P.bix + i], rm = rg[P.bix + i - 1], rp = rg[P.bix + i + 1];
                    pred = r0 > half_vt && r0 > rm && r0 >= rp;
                }
                unsigned long long mask = __ballot(pred);
                while (mask) {
                    const int bpos = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const int im = base + bpos;
                    const double r0 = rg[P.bix + im], rm = rg[P.bix + im - 1], rp = rg[P.bix + im + 1];
                    const double dr = 0.5 * (rp - rm), d2r = 2.0 * r0 - rm - rp;
                    const double fmx = 1.0 / P.dx / ((double)im + dr / d2r);
                    double smx = sinc_wave(rg, ynx, 1.0 / P.dx / fmx + (double)(P.bix + 1), 30, lane);
                    if (smx > 1.0) smx = 1.0 / smx;
                    int place = -1;
                    if (ng < P.maxc) {
                        place = ng++;
                    } else {
                        // weakest candidate so far among 1..maxc-1 (first minimum wins)
                        double ls = c_s - P.octave_cost * (log(P.min_pitch / c_f) * LOG2E_D);
                        int li = hl;
                        if (!mine || hl < 1 || hl >= P.maxc) { ls = 1e300; li = 1 << 20; }
                        for (int off = 32; off > 0; off >>= 1) {
                            const double os = __shfl_xor(ls, off, 64);
                            const int oi = __shfl_xor(li, off, 64);
                            if (os < ls || (os == ls && oi < li)) { ls = os; li = oi; }
                        }
                        double weakest = 2.0;
                        if (ls < weakest) { weakest = ls; place = li; }
                        if (smx - P.octave_cost * (log(P.min_pitch / fmx) * LOG2E_D) <= weakest) place = -1;
                    }
                    if (place >= 0 && mine && hl == place) { c_f = fmx; c_s = smx; c_i = im; }
                }
            }
            if (mine) n = ng;
        }
        if (n > 1) {
            // hand r[-bix..bix] and the candidate lags to k_pitch_refine
            // r is even: only r[0..bix] travels (half the bytes written here and read by k_pitch_refine)
            double *ro = rr_out + fidx * (int64_t)P.rr_half;
            for (int k = hl; k <= P.bix; k += LW) ro[k] = rr[P.bix + k];
            // append to one of RF_LISTS lists: a single counter would serialise ~10^5 returning atomics in L2
            const unsigned int list = (unsigned int)bid & (RF_LISTS - 1);
            unsigned int pos = 0;
            if (hl == 0) pos = atomicAdd(item_count + list * RF_CSTRIDE, (unsigned int)(n - 1));
            pos = __shfl(pos, lane & ~(LW - 1), 64);
            if (hl >= 1 && hl < n) items[(size_t)list * list_cap + pos + hl - 1] = RefineItem{(long long)fidx, hl, c_i};
        }
    }
    // (candidate slots are not cleared: slot 0 is the voiceless candidate by definition and slots >= n are
    //  never read -- k_pitch_delta and k_pitch_path go by ncand)
    if (live && hl == 0) { ncand[fidx] = n; intensity[fidx] = inten; }
    }   // frames of this wavefront
}
