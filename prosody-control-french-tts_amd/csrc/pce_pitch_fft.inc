// pce_pitch_fft.inc -- the fp64 transforms of k_pitch_frames, one wavefront (or half of one) per frame: the Stockham passes through LDS for any N
// (fft_wave) and the three register-resident forms for M = 256, 512 and 1024 complex points with their radix-4/8/16 butterflies, plus the small
// fp64 helpers the pitch kernels share (rcp_f64, cmul_f64, wave_sync).  Included by pce_pitch.hip inside its anonymous namespace.

// ---------------------------------------------------------------------------
// fp64 autocorrelation by FFT, one wavefront per frame, entirely in LDS.
// The zero-padded real frame x[0..N) is read as M = N/2 complex points z[n] = x[2n] + i x[2n+1]
// (the staging buffer IS that array), transformed with Stockham radix-4 (+ one radix-2)
// passes that ping-pong between two LDS buffers, untangled into the power spectrum
// P[k] = |X[k]|^2, re-tangled (P is real and even) and sent through the same forward
// transform again: ac[2n] = Re Y[n], ac[2n+1] = -Im Y[n] (common positive scale dropped;
// it cancels in r[k] = ac[k] / (ac[0] windowR[k])).  Praat itself takes this route
// (NUMfft_forward / power / NUMfft_backward in Sound_to_Pitch.cpp); N = nsampFFT.
// LDS index padding: one complex per 8 keeps the stride-4 Stockham stores conflict-free.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double rcp_f64(double a)
{
    // v_rcp_f64 is good to 2^-24 (measured 4.6e-8); one cubic step r (1 + e + e^2) leaves e^3 ~ 1e-22
    const double r = __builtin_amdgcn_rcp(a);
    const double e = fma(-a, r, 1.0);
    return fma(r, fma(e, e, e), r);
}
__device__ __forceinline__ int ZP(int p) { return p + (p >> 3); }
__device__ __forceinline__ double2 cmul_f64(double2 a, double2 w)
{
    return make_double2(fma(a.x, w.x, -(a.y * w.y)), fma(a.x, w.y, a.y * w.x));
}
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
// forward DFT of M points (exp(-2 pi i ...)); returns the buffer holding the result
__device__ double2 *fft_wave(double2 *src, double2 *dst, int M, const double2 *__restrict__ twM, int lane)
{
    int Ns = 1;
    while (Ns < M) {
        if (M / Ns >= 4) {
            const int nb = M >> 2, tws = M / (Ns << 2);
            for (int b = lane; b < nb; b += 64) {
                const int k = b & (Ns - 1);
                double2 a0 = src[ZP(b)], a1 = src[ZP(b + nb)], a2 = src[ZP(b + 2 * nb)], a3 = src[ZP(b + 3 * nb)];
                if (Ns > 1) {
                    a1 = cmul_f64(a1, twM[k * tws]);
                    a2 = cmul_f64(a2, twM[2 * k * tws]);
                    a3 = cmul_f64(a3, twM[3 * k * tws]);
                }
                const double2 b0 = make_double2(a0.x + a2.x, a0.y + a2.y), b1 = make_double2(a0.x - a2.x, a0.y - a2.y);
                const double2 b2 = make_double2(a1.x + a3.x, a1.y + a3.y);
                const double2 b3 = make_double2(a1.y - a3.y, -(a1.x - a3.x));          // (a1 - a3) * (-i)
                const int base = ((b - k) << 2) + k;
                dst[ZP(base)] = make_double2(b0.x + b2.x, b0.y + b2.y);
                dst[ZP(base + Ns)] = make_double2(b1.x + b3.x, b1.y + b3.y);
                dst[ZP(base + 2 * Ns)] = make_double2(b0.x - b2.x, b0.y - b2.y);
                dst[ZP(base + 3 * Ns)] = make_double2(b1.x - b3.x, b1.y - b3.y);
            }
            Ns <<= 2;
        } else {
            const int nb = M >> 1, tws = M / (Ns << 1);
            for (int b = lane; b < nb; b += 64) {
                const int k = b & (Ns - 1);
                const double2 a0 = src[ZP(b)];
                double2 a1 = src[ZP(b + nb)];
                if (Ns > 1) a1 = cmul_f64(a1, twM[k * tws]);
                const int base = ((b - k) << 1) + k;
                dst[ZP(base)] = make_double2(a0.x + a1.x, a0.y + a1.y);
                dst[ZP(base + Ns)] = make_double2(a0.x - a1.x, a0.y - a1.y);
            }
            Ns <<= 1;
        }
        wave_sync();
        double2 *t = src; src = dst; dst = t;
    }
    return src;
}

// ---------------------------------------------------------------------------
// M = 512 (16 kHz at Praat's 75 Hz floor: N = 1024) keeps the whole transform in registers:
// 512 = 8 x 8 x 8, eight complex points per lane, three radix-8 butterflies per lane and two
// transposes through ONE 9 KB LDS exchange buffer per wavefront.  LDS stores are the scarce
// resource here (ds_write_b128: ~79 B/clk/CU against 256 B/clk for reads), and this form
// stores 40 KB per frame where the ping-pong Stockham passes store ~115 KB; the single buffer
// also doubles the wavefronts a CU can hold.
//   stage 1: lane l holds x[64 a + l]        -> DFT over a, twiddle W512^(l k0)
//   stage 2: lane (c + 8 k0) holds y1[k0][8 b + c] -> DFT over b, twiddle W64^(c k1)
//   stage 3: lane (k0 + 8 k1) holds y2[k0][k1][c]  -> DFT over c: X[k0 + 8 k1 + 64 k2]
// so the result comes back in the layout stage 1 started from (index = lane + 64 r).
// Exchange images: [k0][72] and [c][65] complex: ds_write_b128 (8 contiguous lanes per group,
// 128-byte bank rows) and ds_read_b128 (16-lane groups, 256-byte rows) are both conflict-free.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void dft8_f64(double2 (&a)[8])
{
    const double r = 0.70710678118654752440;
    const double2 b0 = make_double2(a[0].x + a[4].x, a[0].y + a[4].y), b4 = make_double2(a[0].x - a[4].x, a[0].y - a[4].y);
    const double2 b1 = make_double2(a[1].x + a[5].x, a[1].y + a[5].y), t5 = make_double2(a[1].x - a[5].x, a[1].y - a[5].y);
    const double2 b2 = make_double2(a[2].x + a[6].x, a[2].y + a[6].y), t6 = make_double2(a[2].x - a[6].x, a[2].y - a[6].y);
    const double2 b3 = make_double2(a[3].x + a[7].x, a[3].y + a[7].y), t7 = make_double2(a[3].x - a[7].x, a[3].y - a[7].y);
    const double2 b5 = make_double2(r * (t5.x + t5.y), r * (t5.y - t5.x));        // * exp(-i pi/4)
    const double2 b6 = make_double2(t6.y, -t6.x);                                 // * (-i)
    const double2 b7 = make_double2(r * (t7.y - t7.x), -(r * (t7.x + t7.y)));     // * exp(-3 i pi/4)
    const double2 c0 = make_double2(b0.x + b2.x, b0.y + b2.y), c2 = make_double2(b0.x - b2.x, b0.y - b2.y);
    const double2 c1 = make_double2(b1.x + b3.x, b1.y + b3.y), c3 = make_double2(b1.y - b3.y, -(b1.x - b3.x));
    const double2 d0 = make_double2(b4.x + b6.x, b4.y + b6.y), d2 = make_double2(b4.x - b6.x, b4.y - b6.y);
    const double2 d1 = make_double2(b5.x + b7.x, b5.y + b7.y), d3 = make_double2(b5.y - b7.y, -(b5.x - b7.x));
    a[0] = make_double2(c0.x + c1.x, c0.y + c1.y); a[4] = make_double2(c0.x - c1.x, c0.y - c1.y);
    a[2] = make_double2(c2.x + c3.x, c2.y + c3.y); a[6] = make_double2(c2.x - c3.x, c2.y - c3.y);
    a[1] = make_double2(d0.x + d1.x, d0.y + d1.y); a[5] = make_double2(d0.x - d1.x, d0.y - d1.y);
    a[3] = make_double2(d2.x + d3.x, d2.y + d3.y); a[7] = make_double2(d2.x - d3.x, d2.y - d3.y);
}
// forward DFT of 512 points held as z[r] = x[lane + 64 r]; returns X[lane + 64 r] in z[r]
__device__ __forceinline__ void fft512_reg(double2 (&z)[8], double2 *ex, const double2 *tw1 /* [7][64]: W512^(l k) */, const double2 *tw2 /* [7][8]: W64^(c k) */, int lane)
{
    dft8_f64(z);
#pragma unroll
    for (int k = 1; k < 8; k++) z[k] = cmul_f64(z[k], tw1[(k - 1) * 64 + lane]);
#pragma unroll
    for (int k = 0; k < 8; k++) ex[72 * k + lane] = z[k];
    wave_sync();
    const int c = lane & 7, k0 = lane >> 3;
#pragma unroll
    for (int b = 0; b < 8; b++) z[b] = ex[72 * k0 + 8 * b + c];
    wave_sync();
    dft8_f64(z);
#pragma unroll
    for (int k = 1; k < 8; k++) z[k] = cmul_f64(z[k], tw2[(k - 1) * 8 + c]);
#pragma unroll
    for (int k = 0; k < 8; k++) ex[65 * c + k0 + 8 * k] = z[k];
    wave_sync();
#pragma unroll
    for (int q = 0; q < 8; q++) z[q] = ex[65 * q + lane];
    wave_sync();
    dft8_f64(z);
}

// forward DFT of 1024 points (N = 2048: 44.1 kHz at the 150 Hz floor -- the rate of the reference's own recordings)
// by one wavefront, 16 complex points per lane: 1024 = 16 x 8 x 8.
//   stage 1: lane l holds x[64 a + l], a < 16         -> DFT16 over a, twiddle W1024^(l k0)
//   stage 2: lane (c + 8 k0lo) holds y1[k0lo + 8 g][8 b + c]  -> two DFT8 over b, twiddle W64^(c k1)
//   stage 3: lane (k0 + 16 k1lo) holds y2[k0][k1lo + 4 g][c]  -> two DFT8 over c: X[k0 + 16 k1 + 128 k2]
// and the result is back in the input layout (index = lane + 64 r, r = g + 2 k2).  Exchange images [k0][72] and
// [c][129] complex (conflict-free for ds_write_b128 / ds_read_b128 like the 512-point ones).
__device__ __forceinline__ void dft4_f64(double2 &a0, double2 &a1, double2 &a2, double2 &a3)
{
    const double2 t0 = make_double2(a0.x + a2.x, a0.y + a2.y), t1 = make_double2(a0.x - a2.x, a0.y - a2.y);
    const double2 t2 = make_double2(a1.x + a3.x, a1.y + a3.y), t3 = make_double2(a1.y - a3.y, -(a1.x - a3.x));   // (a1 - a3)(-i)
    a0 = make_double2(t0.x + t2.x, t0.y + t2.y); a1 = make_double2(t1.x + t3.x, t1.y + t3.y);
    a2 = make_double2(t0.x - t2.x, t0.y - t2.y); a3 = make_double2(t1.x - t3.x, t1.y - t3.y);
}
__device__ __forceinline__ void dft16_f64(double2 (&x)[16])
{
    // n = 4 n1 + n2: DFT4 over n1, twiddle W16^(n2 k1), DFT4 over n2 -> X[k1 + 4 k2]
    const double c1 = 0.92387953251128675613, s1 = 0.38268343236508977173, r = 0.70710678118654752440;
#pragma unroll
    for (int n2 = 0; n2 < 4; n2++) dft4_f64(x[n2], x[4 + n2], x[8 + n2], x[12 + n2]);       // x[4 k1 + n2] = A[n2][k1]
    auto mulc = [](double2 a, double wr, double wi) { return make_double2(fma(a.x, wr, -(a.y * wi)), fma(a.x, wi, a.y * wr)); };
    x[4 + 1] = mulc(x[4 + 1], c1, -s1);  x[4 + 2] = mulc(x[4 + 2], r, -r);   x[4 + 3] = mulc(x[4 + 3], s1, -c1);     // W16^1, W16^2, W16^3
    x[8 + 1] = mulc(x[8 + 1], r, -r);    x[8 + 2] = make_double2(x[8 + 2].y, -x[8 + 2].x);                           // W16^2, W16^4 = -i
    x[8 + 3] = mulc(x[8 + 3], -r, -r);                                                                             // W16^6
    x[12 + 1] = mulc(x[12 + 1], s1, -c1); x[12 + 2] = mulc(x[12 + 2], -r, -r); x[12 + 3] = mulc(x[12 + 3], -c1, s1); // W16^3, W16^6, W16^9
#pragma unroll
    for (int k1 = 0; k1 < 4; k1++) dft4_f64(x[4 * k1], x[4 * k1 + 1], x[4 * k1 + 2], x[4 * k1 + 3]);   // x[4 k1 + k2] = X[k1 + 4 k2]
    // to natural order X[k] at x[k]: transpose the 4 x 4 index (k1, k2) -> (k2, k1)
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i + 1; j < 4; j++) { const double2 t = x[4 * i + j]; x[4 * i + j] = x[4 * j + i]; x[4 * j + i] = t; }
}
__device__ __forceinline__ void fft1024_reg(double2 (&z)[16], double2 *ex, const double2 *tw1 /* [15][64]: W1024^(l k) */,
                                            const double2 *tw2 /* [7][8]: W64^(c k) */, int lane)
{
    dft16_f64(z);
#pragma unroll
    for (int k = 1; k < 16; k++) z[k] = cmul_f64(z[k], tw1[(k - 1) * 64 + lane]);
#pragma unroll
    for (int k = 0; k < 16; k++) ex[72 * k + lane] = z[k];
    wave_sync();
    const int c = lane & 7, k0lo = lane >> 3;
#pragma unroll
    for (int g = 0; g < 2; g++)
#pragma unroll
        for (int b = 0; b < 8; b++) z[8 * g + b] = ex[72 * (k0lo + 8 * g) + 8 * b + c];
    wave_sync();
    {
        double2 h0[8], h1[8];
#pragma unroll
        for (int b = 0; b < 8; b++) { h0[b] = z[b]; h1[b] = z[8 + b]; }
        dft8_f64(h0); dft8_f64(h1);
#pragma unroll
        for (int k = 1; k < 8; k++) { const double2 w = tw2[(k - 1) * 8 + c]; h0[k] = cmul_f64(h0[k], w); h1[k] = cmul_f64(h1[k], w); }
#pragma unroll
        for (int k = 0; k < 8; k++) { ex[129 * c + k0lo + 16 * k] = h0[k]; ex[129 * c + k0lo + 8 + 16 * k] = h1[k]; }
    }
    wave_sync();
    {
        double2 h0[8], h1[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { h0[q] = ex[129 * q + lane]; h1[q] = ex[129 * q + 64 + lane]; }
        wave_sync();
        dft8_f64(h0); dft8_f64(h1);
#pragma unroll
        for (int k2 = 0; k2 < 8; k2++) { z[2 * k2] = h0[k2]; z[2 * k2 + 1] = h1[k2]; }
    }
}

// forward DFT of 256 points by a HALF wavefront (two frames per wavefront): 256 = 8 x 8 x 4,
// z[r] = x[hl + 32 r] in, X[hl + 32 r] out, hl = lane within the half.  Exchange images
// [k0][36] and [c][66] complex in this frame's 288-complex region (conflict-free as above).
__device__ __forceinline__ void fft256_half(double2 (&z)[8], double2 *ex, const double2 *tw1 /* [7][32]: W256^(l k) */, const double2 *tw2 /* [7][4]: W32^(c k) */, int hl)
{
    dft8_f64(z);
#pragma unroll
    for (int k = 1; k < 8; k++) z[k] = cmul_f64(z[k], tw1[(k - 1) * 32 + hl]);
#pragma unroll
    for (int k = 0; k < 8; k++) ex[36 * k + hl] = z[k];
    wave_sync();
    const int c = hl & 3, k0 = hl >> 2;
#pragma unroll
    for (int b = 0; b < 8; b++) z[b] = ex[36 * k0 + 4 * b + c];
    wave_sync();
    dft8_f64(z);
#pragma unroll
    for (int k = 1; k < 8; k++) z[k] = cmul_f64(z[k], tw2[(k - 1) * 4 + c]);
#pragma unroll
    for (int k = 0; k < 8; k++) ex[66 * c + k0 + 8 * k] = z[k];
    wave_sync();
    double2 v[2][4];
#pragma unroll
    for (int g = 0; g < 2; g++)
#pragma unroll
        for (int q = 0; q < 4; q++) v[g][q] = ex[66 * q + 32 * g + hl];
    wave_sync();
#pragma unroll
    for (int g = 0; g < 2; g++) {
        const double2 t0 = make_double2(v[g][0].x + v[g][2].x, v[g][0].y + v[g][2].y), t1 = make_double2(v[g][0].x - v[g][2].x, v[g][0].y - v[g][2].y);
        const double2 t2 = make_double2(v[g][1].x + v[g][3].x, v[g][1].y + v[g][3].y), t3 = make_double2(v[g][1].y - v[g][3].y, -(v[g][1].x - v[g][3].x));
        z[g] = make_double2(t0.x + t2.x, t0.y + t2.y);     z[2 + g] = make_double2(t1.x + t3.x, t1.y + t3.y);
        z[4 + g] = make_double2(t0.x - t2.x, t0.y - t2.y); z[6 + g] = make_double2(t1.x - t3.x, t1.y - t3.y);
    }
}
