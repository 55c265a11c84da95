// pce_pitch_refine.inc -- k_pitch_refine and its polynomial trigonometry and group-wide sinc interpolations.  Included by pce_pitch.hip after
// pce_pitch_fft.inc (rcp_f64).

// ---------------------------------------------------------------------------
// k_pitch_refine: Praat's second pass (NUMimproveMaximum, sinc depth 70/700) over the flat
// list of candidates.  Eight lanes per candidate: the 144 autocorrelation values a
// depth-70 interpolation can touch live in registers (18 per lane, fixed absolute indices),
// the per-evaluation scalars (Brent state, sin) are shared by eight candidates per wave, and
// the 8-lane sums use DPP row operations (no LDS).  Trigonometry is evaluated with plain
// polynomials (every argument is known to lie in (0, pi]); along a lane's rows the raised-cosine
// arguments form an arithmetic progression, so only the two rows nearest x on each side take
// the polynomial and the rest follow by the three-term cosine recurrence.
// ---------------------------------------------------------------------------
// cos(h) and sin(h) for h in [0, pi/2] (Taylor about 0; truncation < 1e-19), evaluated by Estrin's
// scheme: a dependent fp64 FMA costs ~30 cycles on this part (measured), so the 13-deep Horner chain
// was the critical path of every evaluation; this form is 5 deep for two more multiplies.
__device__ __forceinline__ double poly13_estrin(double z, double c0, double c1, double c2, double c3, double c4, double c5, double c6,
                                                double c7, double c8, double c9, double c10, double c11, double c12)
{
    const double z2 = z * z, z4 = z2 * z2, z8 = z4 * z4;
    const double q0 = fma(c1, z, c0), q1 = fma(c3, z, c2), q2 = fma(c5, z, c4), q3 = fma(c7, z, c6), q4 = fma(c9, z, c8), q5 = fma(c11, z, c10);
    const double r0 = fma(q1, z2, q0), r1 = fma(q3, z2, q2), r2 = fma(q5, z2, q4);
    const double s0 = fma(r1, z4, r0), s1 = fma(c12, z4, r2);
    return fma(s1, z8, s0);
}
__device__ __forceinline__ double cos_q(double h)
{
    return poly13_estrin(h * h, 1.0, -0.5, 4.1666666666666664e-02, -1.3888888888888889e-03, 2.4801587301587302e-05, -2.7557319223985888e-07,
                         2.0876756987868099e-09, -1.1470745597729725e-11, 4.7794773323873853e-14, -1.5619206968586225e-16,
                         4.1103176233121648e-19, -8.8967913924505741e-22, 1.6117375710961184e-24);
}
__device__ __forceinline__ double sin_q(double h)
{
    // sin h = h + h z (s0 + s1 z + ... + s11 z^11), z = h^2
    const double z = h * h;
    const double z2 = z * z, z4 = z2 * z2, z8 = z4 * z4;
    const double q0 = fma(8.3333333333333332e-03, z, -1.6666666666666666e-01), q1 = fma(2.7557319223985893e-06, z, -1.9841269841269841e-04);
    const double q2 = fma(1.6059043836821613e-10, z, -2.5052108385441720e-08), q3 = fma(2.8114572543455206e-15, z, -7.6471637318198164e-13);
    const double q4 = fma(1.9572941063391263e-20, z, -8.2206352466243295e-18), q5 = -3.8681701706306841e-23;
    const double r0 = fma(q1, z2, q0), r1 = fma(q3, z2, q2), r2 = fma(q5, z2, q4);
    const double p = fma(r2, z8, fma(r1, z4, r0));
    return fma(p * z, h, h);
}
__device__ __forceinline__ double sin_0pi(double a) { const double h = 0.5 * a; return 2.0 * sin_q(h) * cos_q(h); }
__device__ __forceinline__ double one_plus_cos_0pi(double a) { const double c = cos_q(0.5 * a); return 2.0 * c * c; }

// NUM_interpolate_sinc for a depth that stays inside the register window.
// yv[m] = y[wbase + l8 + 8 m] (1-based y index), m < 18; the caller guarantees 8 <= D and that
// midleft is ixmid-1 or ixmid with wbase = ixmid - 71, so window rows m <= 7 lie left of x,
// rows m >= 9 right of it and only row 8 straddles it.  Per lane the index distance k
// changes by 8 from row to row: the (-1)^k sign is one value per side.  sin(pi (1 - t)) is
// taken equal to sin(pi t) (Praat evaluates both; they differ by rounding only).
// The window factor 1 + cos(aa_k), aa_k = pi (k + frac) / (D + frac), is linear in k: with
// u_m = 1 + cos(aa0 + m delta), u_(m+1) = tc u_m - u_(m-1) + (2 - tc), tc = 2 cos(delta).
// Rows are walked outward from x, so a row inside the depth limit only ever depends on rows
// inside it (rows beyond the limit are discarded by the k < D select, whatever they hold).
__device__ __forceinline__ double sinc_w(double kd, double a0, double yu /* y (1 + cos) */)
{
    return yu * rcp_f64(fma(kd, PI_D, a0));         // the side's +-0.5 sin factor is applied once per side
}
// G lanes per candidate, NR = 144 / G rows per lane; row RS straddles x, rows < RS lie left, rows > RS right.
template <int G>
__device__ __forceinline__ double sinc_group_reg(const double (&yv)[144 / G], int wbase, int ynx, double x, int maxDepth, int lg)
{
    constexpr int NR = 144 / G, RS = (72 - G) / G;
    const int midleft = (int)floor(x), midright = midleft + 1;
    if (x == (double)midleft) {
        double pick = 0.0;
#pragma unroll
        for (int m = 0; m < NR; m++) if (wbase + lg + G * m == midleft) pick = yv[m];
        return dpp_row_sum<G>(pick);
    }
    int D = maxDepth;
    if (D > midright - 1) D = midright - 1;
    if (D > ynx - midleft) D = ynx - midleft;
    const double dlim = (double)D;
    const int left = midright - D, right = midleft + D;
    const double a_l = PI_D * (x - (double)midleft), a_r = PI_D * ((double)midright - x);
    // sin(pi f) = sin(pi (1 - f)): fold to [0, pi/2] and take ONE polynomial (sin_0pi costs a sine and a cosine)
    const double hs = 0.5 * sin_q(fmin(a_l, a_r));
    const double rden_l = rcp_f64(x - (double)left + 1.0), rden_r = rcp_f64((double)right - x + 1.0);
    const double aa_l = a_l * rden_l, daa_l = PI_D * rden_l;
    const double aa_r = a_r * rden_r, daa_r = PI_D * rden_r;
    const int kl0 = midleft - wbase - lg;             // k of row 0 on the left side (decreases by G per row)
    const int kr0 = wbase + lg - midright;            // k of row 0 on the right side (increases by G per row)
    const double hs_l = (kl0 & 1) ? -hs : hs, hs_r = (kr0 & 1) ? -hs : hs;
    const double kdl = (double)kl0, kdr = (double)kr0;
    // rows < RS and > RS have k >= 0 by construction (wbase = ixmid - 71): only the depth limit can drop them
    auto keep = [&](double kd, double t) { return kd < dlim ? t : 0.0; };
    double acc;
    {   // row RS holds the lanes around x
        const bool is_left = kl0 - G * RS >= 0;
        const double kd = is_left ? kdl - (double)(G * RS) : kdr + (double)(G * RS);
        const double u = one_plus_cos_0pi(fma(kd, is_left ? daa_l : daa_r, is_left ? aa_l : aa_r));
        const double ts = (is_left ? hs_l : hs_r) * sinc_w(kd, is_left ? a_l : a_r, yv[RS] * u);
        acc = (kd >= 0.0 && kd < dlim) ? ts : 0.0;
    }
    // Two rows share one reciprocal: t0/a0 + t1/a1 = (t0 a1 + t1 a0) / (a0 a1) (a = pi (k + frac) > 0; a v_rcp_f64
    // issues at quarter rate), so the rows are first collected (masked numerators t = y (1 + cos), denominators a)
    // and then folded in pairs.
    {   // left side, rows RS-1 (nearest x) .. 0
        constexpr int NL = RS;
        double tv[NL], av[NL];
        const double cq = cos_q(0.5 * G * daa_l);                       // cos(delta / 2), delta = G daa <= pi
        const double tc = fma(4.0 * cq, cq, -2.0), g = 2.0 - tc;
        const double k1 = kdl - (double)(G * (RS - 1)), k0 = kdl - (double)(G * (RS - 2));
        double u1 = one_plus_cos_0pi(fma(k1, daa_l, aa_l));
        double u0 = one_plus_cos_0pi(fma(k0, daa_l, aa_l));
        tv[0] = keep(k1, yv[RS - 1] * u1); av[0] = fma(k1, PI_D, a_l);
        tv[1] = keep(k0, yv[RS - 2] * u0); av[1] = fma(k0, PI_D, a_l);
#pragma unroll
        for (int m = RS - 3; m >= 0; m--) {
            const double u = fma(tc, u0, g - u1);        // (g - u1) is off the critical path
            u1 = u0; u0 = u;
            const double kd = kdl - (double)(G * m);
            tv[RS - 1 - m] = keep(kd, yv[m] * u); av[RS - 1 - m] = fma(kd, PI_D, a_l);
        }
        double side = 0.0;
#pragma unroll
        for (int q = 0; q + 1 < NL; q += 2) side += fma(tv[q], av[q + 1], tv[q + 1] * av[q]) * rcp_f64(av[q] * av[q + 1]);
        if (NL & 1) side += tv[NL - 1] * rcp_f64(av[NL - 1]);
        acc = fma(hs_l, side, acc);
    }
    {   // right side, rows RS+1 (nearest x) .. NR-1
        constexpr int NRt = NR - RS - 1;
        double tv[NRt], av[NRt];
        const double cq = cos_q(0.5 * G * daa_r);
        const double tc = fma(4.0 * cq, cq, -2.0), g = 2.0 - tc;
        const double k1 = kdr + (double)(G * (RS + 1)), k0 = kdr + (double)(G * (RS + 2));
        double u1 = one_plus_cos_0pi(fma(k1, daa_r, aa_r));
        double u0 = one_plus_cos_0pi(fma(k0, daa_r, aa_r));
        tv[0] = keep(k1, yv[RS + 1] * u1); av[0] = fma(k1, PI_D, a_r);
        tv[1] = keep(k0, yv[RS + 2] * u0); av[1] = fma(k0, PI_D, a_r);
#pragma unroll
        for (int m = RS + 3; m < NR; m++) {
            const double u = fma(tc, u0, g - u1);        // (g - u1) is off the critical path
            u1 = u0; u0 = u;
            const double kd = kdr + (double)(G * m);
            tv[m - RS - 1] = keep(kd, yv[m] * u); av[m - RS - 1] = fma(kd, PI_D, a_r);
        }
        double side = 0.0;
#pragma unroll
        for (int q = 0; q + 1 < NRt; q += 2) side += fma(tv[q], av[q + 1], tv[q + 1] * av[q]) * rcp_f64(av[q] * av[q + 1]);
        if (NRt & 1) side += tv[NRt - 1] * rcp_f64(av[NRt - 1]);
        acc = fma(hs_r, side, acc);
    }
    return dpp_row_sum<G>(acc);
}

// generic NUM_interpolate_sinc with y in global memory (depth 700, or windows near the array ends)
template <int G> __device__ double sinc_group_mem(const double *__restrict__ yh /* r[0..bix] */, int ynx, double x, int maxDepth, int lg)
{
    const int mid = (ynx + 1) >> 1;                      // Praat's y(i) = r[i - mid] = yh[|i - mid|]
    auto Y = [&](int i) { return yh[abs(i - mid)]; };
    const int midleft = (int)floor(x), midright = midleft + 1;
    if (x > (double)ynx) return Y(ynx);
    if (x < 1.0) return Y(1);
    if (x == (double)midleft) return Y(midleft);
    if (maxDepth > midright - 1) maxDepth = midright - 1;
    if (maxDepth > ynx - midleft) maxDepth = ynx - midleft;
    if (maxDepth <= 0) return Y((int)floor(x + 0.5));
    if (maxDepth == 1) return Y(midleft) + (x - (double)midleft) * (Y(midright) - Y(midleft));
    if (maxDepth == 2) {
        const double yl = Y(midleft), yr = Y(midright);
        const double dyl = 0.5 * (yr - Y(midleft - 1)), dyr = 0.5 * (Y(midright + 1) - yl);
        const double fil = x - (double)midleft, fir = (double)midright - x;
        return yl * fir + yr * fil - fil * fir * (0.5 * (dyr - dyl) + (fil - 0.5) * (dyl + dyr - 2.0 * (yr - yl)));
    }
    const int left = midright - maxDepth, right = midleft + maxDepth;
    const double a_l = PI_D * (x - (double)midleft), a_r = PI_D * ((double)midright - x);
    const double hs_l = 0.5 * sin_0pi(a_l), hs_r = 0.5 * sin_0pi(a_r);
    const double den_l = x - (double)left + 1.0, den_r = (double)right - x + 1.0;
    const double aa_l = a_l / den_l, daa_l = PI_D / den_l;
    const double aa_r = a_r / den_r, daa_r = PI_D / den_r;
    double acc = 0.0;
    for (int t = lg; t < 2 * maxDepth; t += G) {
        const bool is_left = t < maxDepth;
        const int k = is_left ? t : t - maxDepth;
        const double kd = (double)k;
        const double a = fma(kd, PI_D, is_left ? a_l : a_r);
        const double aa = fma(kd, is_left ? daa_l : daa_r, is_left ? aa_l : aa_r);
        double hs = is_left ? hs_l : hs_r;
        if (k & 1) hs = -hs;
        const int ix = is_left ? midleft - k : midright + k;
        acc += Y(ix) * (hs * rcp_f64(a) * one_plus_cos_0pi(aa));
    }
    return dpp_row_sum<G>(acc);
}

template <int G>
__global__ __launch_bounds__(256, G == 8 ? 3 : 2) void k_pitch_refine(PiParams P, const double *__restrict__ rr_in, const RefineItem *__restrict__ items,
                                                     const unsigned int *__restrict__ item_count, unsigned int list_cap,
                                                     double *__restrict__ cand)
{
    constexpr int NR = 144 / G, GS = G == 8 ? 3 : 2;
    const int l8 = threadIdx.x & (G - 1);
    const unsigned int gid = (blockIdx.x * blockDim.x + threadIdx.x) >> GS;
    const unsigned int list = gid & (RF_LISTS - 1);
    const unsigned int group = gid / RF_LISTS;
    const unsigned int n_groups = ((gridDim.x * blockDim.x) >> GS) / RF_LISTS;
    const unsigned int count = item_count[list * RF_CSTRIDE];
    items += (size_t)list * list_cap;
    const int ynx = 2 * P.bix + 1;
    const double golden = 1.0 - 0.6180339887498948482045868343656381177203;
    const double tol = 1e-10;
    auto finish = [&](const RefineItem &item, double xres, double yres) {
        xres -= (double)(P.bix + 1);
        if (yres > 1.0) yres = 1.0 / yres;
        if (l8 == 0) {
            cand[item.frame * 32 + item.slot] = 1.0 / P.dx / xres;
            cand[item.frame * 32 + 16 + item.slot] = yres;
        }
    };
    // The maximiser as a state machine: every trip of the loop is ONE function evaluation for each of the wave's eight candidates, and a
    // group whose candidate has converged fetches its next item at once, so candidates with different iteration counts do not wait for
    // one another.  Two searches (round 3):
    //   * successive parabolic interpolation seeded with the three samples around the maximum (their function values are the
    //     autocorrelation samples themselves: no evaluation): the first trial point already is the parabolic estimate, and the fit through
    //     the best three points converges superlinearly: 3-4 evaluations (stop: a step below 3e-8 |x| after a step below 1e-3).
    //     Praat's NUMminimize_brent (a golden-section opening of [ixmid - 1, ixmid + 1], then a bracket that has to close to 1.5e-8 |x|
    //     from both sides) takes 9-18 for the same maximum, whose position it reports within that tolerance.  |x| is the position in the
    //     array r[-bix..bix], lag + bix + 1, not the lag: the reference's answer is determined to 2 x 1.5e-8 (lag + bix + 1) lags, which is
    //     3e-8 (1 + (bix + 1) / lag) relative in F0, against a parity gate of 1e-6 (REFINE_PARITY_REL);
    //   * Praat's own iterates, exactly as before, for the candidates where the two could differ by more than rounding: the
    //     interpolant is smooth on either side of the sample ixmid but has a kink AT it (the sinc window changes with floor(x)), so a
    //     maximum within a few thousandths of a lag of the sample can split into one local maximum per side (measured on synthetic
    //     autocorrelations: discrepancies of 2e-5 .. 7e-5 relative, all within 0.007 lags of the sample) and which one the reference
    //     reports depends on its path.  Every candidate whose parabolic search ends within 0.03 lags of the sample (3 %), or fails a
    //     safeguard (step outside the bracket, no convergence in 10 steps), is searched again the reference's way.  So is, at once, every
    //     candidate of a lag so short that the two tolerances together ((2 x 1.5e-8 + 3e-8) |x|) exceed the gate: lag < 0.06 (lag + bix + 1),
    //     which with bix = 1.5 periods of the floor is a frequency above 10.5 x the floor (lags below 11 at 16 kHz / 150 Hz, below 92 at
    //     48 kHz / 50 Hz; tests/test_gpu_pitch_stages.py measured up to 5.1e-6 relative on such candidates before).  At the floors in use
    //     they lie above the ceiling, or just under it at 50 Hz: voiceless to the path finder, which never reads their frequency.
    // Elsewhere the maximum in the bracket is unique, both searches end within their tolerance of it, and the strengths agree to second
    // order (the maximum is flat).  PCE_PITCH_REFINE=praat runs every candidate the reference's way.
    unsigned int it = group;
    bool have = false;
    RefineItem item = {0, 0, 0};
    const double *y = rr_in;
    int wbase = 0, depth = 70, iter = 0;             // iter >= 0: Brent's iteration count; iter < 0: parabolic search, -1 - evaluations so far
    bool fast = false;
    double yv[NR];
    double a = 0.0, b = 0.0, v = 0.0, w = 0.0, x = 0.0, fv = 0.0, fw = 0.0, fx = 0.0, t = 0.0, prev_step = 1.0;
    const double sqrt_epsilon = 1.4901161193847656e-08, spi_stop = P.refine_tol_rel;
    constexpr double REFINE_PARITY_REL = 1e-6;         // what the seeded mode promises of a candidate's frequency against the reference's (include/pce.h)
    // Brent's choice of the next trial point from the state (a, b, x, w, v); true: converged
    auto brent_next = [&]() -> bool {
        const double range = b - a;
        const double middle_range = (a + b) / 2.0;
        const double tol_act = sqrt_epsilon * fabs(x) + tol / 3.0;
        if (fabs(x - middle_range) + range / 2.0 <= 2.0 * tol_act) return true;
        double new_step = golden * (x < middle_range ? b - x : a - x);
        if (fabs(x - w) >= tol_act) {
            double tt = (x - w) * (fx - fv);
            double q = (x - v) * (fx - fw);
            double p = (x - v) * q - (x - w) * tt;
            q = 2.0 * (q - tt);
            if (q > 0.0) p = -p; else q = -q;
            if (fabs(p) < fabs(new_step * q) && p > q * (a - x + 2.0 * tol_act) && p < q * (b - x - 2.0 * tol_act))
                new_step = p * rcp_f64(q);          // (an IEEE divide is ~35 instructions; this is within 1 ulp of it)
        }
        if (fabs(new_step) < tol_act) new_step = new_step > 0.0 ? tol_act : -tol_act;
        t = x + new_step;
        return false;
    };
    auto brent_start = [&](double node) {
        a = node - 1.0; b = node + 1.0;
        v = a + golden * (b - a);
        t = v; iter = 0;
    };
    // next point of the parabolic search: 0 = evaluate t, 1 = converged at x, 2 = leave it to Brent
    auto spi_next = [&]() -> int {
        const double tt = (x - w) * (fx - fv);
        double q = (x - v) * (fx - fw);
        double p = (x - v) * q - (x - w) * tt;
        q = 2.0 * (q - tt);
        if (q == 0.0) return 2;
        if (q > 0.0) p = -p; else q = -q;
        const double step = p * rcp_f64(q), tn = x + step;
        if (!(tn > a && tn < b)) return 2;
        const int n_eval = -1 - iter;
        if (n_eval >= 2 && fabs(step) <= spi_stop * fabs(x) && fabs(prev_step) <= 1e-3) return 1;
        if (n_eval >= 10) return 2;
        prev_step = step; t = tn;
        return 0;
    };
    // a group's next item is fetched one item ahead and the 21 autocorrelation values of an item are requested together: one memory
    // round trip per item stands in the wave's instruction stream, not three
    RefineItem nxt = {0, 0, 0};
    if (it < count) nxt = items[it];
    for (;;) {
        while (!have && it < count) {
            item = nxt;
            it += n_groups;
            if (it < count) nxt = items[it];
            y = rr_in + item.frame * (long long)P.rr_half;               // Praat's y(i) = r[i - mid] = y[|i - mid|], mid = bix + 1
            const int ixmid = item.imax + P.bix + 1;
            if (ixmid <= 1) { finish(item, 1.0, y[P.bix]); continue; }
            if (ixmid >= ynx) { finish(item, (double)ynx, y[P.bix]); continue; }
            // depth choice uses the first-pass (parabolic) frequency, as Praat does
            const double r0 = y[abs(item.imax)], rm = y[abs(item.imax - 1)], rp = y[abs(item.imax + 1)];
            const double dr = 0.5 * (rp - rm), d2r = 2.0 * r0 - rm - rp;
            const double f1 = 1.0 / P.dx / ((double)item.imax + dr / d2r);
            depth = f1 > 0.3 / P.dx ? 700 : 70;
            // the register window serves midleft in {ixmid-1, ixmid}: needs depth <= 70 and D >= 8 for both
            fast = depth == 70 && ixmid - 1 >= 9 && ynx - ixmid >= 8;
            wbase = ixmid - 71;
#pragma unroll
            for (int m = 0; m < NR; m++) {                                 // (loaded whether or not the fast path will use them)
                const int ix = wbase + l8 + G * m;
                yv[m] = (ix >= 1 && ix <= ynx) ? y[abs(ix - P.bix - 1)] : 0.0;
            }
            have = true;
            if (P.refine_seeded && (2.0 * sqrt_epsilon + spi_stop) * (double)ixmid <= REFINE_PARITY_REL * (double)item.imax) {
                // the interpolant passes through the samples: f(ixmid) = -r0, f(ixmid -+ 1) = -rm / -rp
                a = (double)(ixmid - 1); b = (double)(ixmid + 1);
                x = (double)ixmid; fx = -r0;
                if (rm >= rp) { w = a; fw = -rm; v = b; fv = -rp; } else { w = b; fw = -rp; v = a; fv = -rm; }
                iter = -1; prev_step = 1.0;
                if (spi_next() != 0) brent_start((double)ixmid);
            } else brent_start((double)ixmid);
        }
        if (__ballot(have) == 0) break;
        if (have) {
            const double ft = fast ? -sinc_group_reg<G>(yv, wbase, ynx, t, 70, l8) : -sinc_group_mem<G>(y, ynx, t, depth, l8);
            if (iter == 0) {
                x = v; w = v; fx = ft; fw = ft; fv = ft;
            } else if (ft <= fx) {
                if (t < x) b = x; else a = x;
                v = w; w = x; x = t;
                fv = fw; fw = fx; fx = ft;
            } else {
                if (t < x) a = t; else b = t;
                if (ft <= fw || w == x) { v = w; w = t; fv = fw; fw = ft; }
                else if (ft <= fv || v == x || v == w) { v = t; fv = ft; }
            }
            if (iter >= 0) {
                iter++;
                if (iter > 60 || brent_next()) { finish(item, x, -fx); have = false; }
            } else {
                iter--;
                const double node = (double)(item.imax + P.bix + 1);
                const int r = spi_next();
                if (r == 1 && fabs(x - node) >= 0.03) { finish(item, x, -fx); have = false; }
                else if (r != 0) brent_start(node);
            }
        }
    }
}
