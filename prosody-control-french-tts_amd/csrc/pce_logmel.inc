// pce_logmel.inc -- the log-mel kernels k_logmel_frames and k_logmel_norm (included by pce_whisper_impl.inc inside its anonymous namespace).
// ---------------------------------------------------------------------------
// log-mel
// ---------------------------------------------------------------------------
struct MelTables {            // device pointers
    const float2 *w16;        // [16]      exp(-2 pi i m / 16)
    const float2 *w400;       // [25][16]  exp(-2 pi i n2 k1 / 400)
    const float2 *w25;        // [25]      exp(-2 pi i m / 25)
    const float *window;      // [400]     periodic Hann
    const int *mel_lo;        // [n_mels]  first bin of band
    const int *mel_n;         // [n_mels]  number of bins
    const int *mel_off;       // [n_mels]  offset into mel_w
    const float *mel_w;       // packed weights
    int mel_total;            // number of packed weights (<= LM_MELW)
};

__device__ __forceinline__ unsigned int f32_order_key(float f)
{
    const unsigned int b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float f32_from_key(unsigned int k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// frame0 == nullptr: the window is frames 0..2999 of the clip trimmed to 30 s (pad_or_trim + log_mel_spectrogram).
// frame0 != nullptr: whisper.transcribe's slicing of the log-mel of the WHOLE clip followed by 30 s of zeros: the window is
// frames frame0[clip] .. +2999, samples beyond 30 s exist, and (scan != 0) a first launch reduces the maximum over every
// frame that overlaps audio (the frames of pure padding are at the -10 floor) without writing anything.
constexpr int LM_MELW = 1024;             // packed mel weights k_logmel_frames keeps in LDS (80 bands: 404, 128 bands: 406)
// PCE_NO_PK_F32 (pce_internal.h): this kernel is compiled WITHOUT packed fp32 instructions.  The complex products below make the compiler
// form v_pk_mul_f32 / v_pk_add_f32 with op_sel:[0,1], and that selection returns wrong values in lanes 48..63 whenever another wave on the
// same SIMD executes MFMA -- the encoder of another process or of another stream (profiles/r06/multiprocess_glitch.txt: a frame of a clip's
// log-mel off now and then with three processes on one device; tools/lab/pk_victim.hip is the reduced case).  Same operations, same order, same bits.
template <int LM_G>                       // frames a wave processes before it writes their values (LM_G * 4 bytes per band and store)
__global__ __launch_bounds__(256) PCE_NO_PK_F32 void k_logmel_frames(const int16_t *__restrict__ pcm, const int64_t *__restrict__ clip_off, int n_mels,
                                                      MelTables T, float *__restrict__ logspec /* [clip][n_mels][3000] */,
                                                      unsigned int *__restrict__ clip_max, const int64_t *__restrict__ frame0, int scan)
{
    __shared__ float xs[4][W_NFFT];
    __shared__ float2 ys[4][25 * 16];
    __shared__ float pw[4][W_BINS + 3];
    __shared__ float2 s_w16[16], s_w25[25], s_w400[25 * 16];
    __shared__ float s_melw[LM_MELW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < T.mel_total; i += 256) s_melw[i] = T.mel_w[i];
    for (int i = tid; i < 16; i += 256) s_w16[i] = T.w16[i];
    for (int i = tid; i < 25; i += 256) s_w25[i] = T.w25[i];
    for (int i = tid; i < 400; i += 256) s_w400[i] = T.w400[i];
    __syncthreads();
    const int clip = blockIdx.y;
    const int64_t base = clip_off[clip], full = clip_off[clip + 1] - base;
    const int64_t len = frame0 ? full : min<int64_t>(full, (int64_t)W_SAMPLES);
    const int64_t f_begin = (frame0 && !scan) ? frame0[clip] : 0;
    const int64_t n_fr = scan ? (full + W_NFFT / 2) / W_HOP + 1 : W_FRAMES;       // scan: every frame that can see a sample
    // loop invariants of a lane (round 5: they were global loads inside the frame loop -- the band loop's were dependent ones, a latency chain of
    // up to 34 L2 round trips per frame): its seven window taps, the extent of its (up to two) mel bands
    float win[7];
#pragma unroll
    for (int i = 0; i < 7; i++) win[i] = (lane + 64 * i) < W_NFFT ? T.window[lane + 64 * i] : 0.f;
    int b_lo[2], b_cnt[2], b_off[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int b = lane + 64 * i;
        b_lo[i] = b < n_mels ? T.mel_lo[b] : 0; b_cnt[i] = b < n_mels ? T.mel_n[b] : 0; b_off[i] = b < n_mels ? T.mel_off[b] : 0;
    }
    float vmax = -1e30f;
    // A wave takes LM_G consecutive frames at a time and hands their log-mel values over through LDS, so that a band's row leaves as one
    // 64-byte segment per group (round 5: one 4-byte store per band and frame, 3 000 floats apart, was a read-modify-write of a sector each --
    // 4 x the kernel's algorithmic traffic in the PMC pass of round 4)
    extern __shared__ float lm_ob[];                              // [4 waves][n_mels][LM_G + 1]
    float *ob = lm_ob + (size_t)wv * n_mels * (LM_G + 1);
    const int64_t n_groups = (n_fr + LM_G - 1) / LM_G;
    for (int64_t gi = blockIdx.x * 4 + wv; gi < n_groups; gi += gridDim.x * 4) {
      for (int j = 0; j < LM_G; j++) {
        const int64_t fl = gi * LM_G + j;
        if (fl >= n_fr) break;
        const int64_t frame = f_begin + fl;
        if (frame * W_HOP - W_NFFT / 2 >= len) {
            // a frame of the zero padding behind the audio (two thirds of the 30 s window of a 10 s clip): every sample is an exact zero, so are
            // the spectrum and the mel energies, and the value is log10 of the 1e-10 clamp -- written without running the transform
            const float lg = log10f(fmaxf(0.f, 1e-10f));
            for (int b = lane; b < n_mels; b += 64) ob[b * (LM_G + 1) + j] = lg;
            vmax = fmaxf(vmax, lg);
            continue;
        }
        // windowed frame, centre = frame*160, reflect padding at the start, zeros past the audio
#pragma unroll
        for (int wi = 0; wi < 7; wi++) {
            const int n = lane + 64 * wi;
            if (n < W_NFFT) {
                int64_t i = frame * W_HOP - W_NFFT / 2 + n;
                if (i < 0) i = -i;
                const float v = (i < len) ? (float)pcm[base + i] * (1.0f / 32768.0f) : 0.0f;
                xs[wv][n] = v * win[wi];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
        // stage A: Y[n2][k1] = sum_{n1<16} x[25 n1 + n2] W16^{n1 k1}, then twiddle W400^{n2 k1}
        for (int o = lane; o < 400; o += 64) {
            const int n2 = o >> 4, k1 = o & 15;
            float re = 0.f, im = 0.f;
#pragma unroll
            for (int n1 = 0; n1 < 16; n1++) {
                const float x = xs[wv][25 * n1 + n2];
                const float2 w = s_w16[(n1 * k1) & 15];
                re = fmaf(x, w.x, re); im = fmaf(x, w.y, im);
            }
            const float2 t = s_w400[o];
            ys[wv][o] = make_float2(re * t.x - im * t.y, re * t.y + im * t.x);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
        // stage B: X[k1 + 16 k2] = sum_{n2<25} Y[n2][k1] W25^{n2 k2}; only k <= 200 is needed
        for (int k = lane; k < W_BINS; k += 64) {
            const int k1 = k & 15, k2 = k >> 4;
            float re = 0.f, im = 0.f;
            int m = 0;
            for (int n2 = 0; n2 < 25; n2++) {
                const float2 y = ys[wv][n2 * 16 + k1];
                const float2 w = s_w25[m];
                re += y.x * w.x - y.y * w.y; im += y.x * w.y + y.y * w.x;
                m += k2; if (m >= 25) m -= 25;
            }
            pw[wv][k] = re * re + im * im;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int bi = 0; bi < 2; bi++) {
            const int b = lane + 64 * bi;
            if (b < n_mels) {
                const int lo = b_lo[bi], cnt = b_cnt[bi];
                const float *w = s_melw + b_off[bi];
                float acc = 0.f;
                for (int i = 0; i < cnt; i++) acc = fmaf(w[i], pw[wv][lo + i], acc);
                const float lg = log10f(fmaxf(acc, 1e-10f));
                ob[b * (LM_G + 1) + j] = lg;
                vmax = fmaxf(vmax, lg);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
      // (round 6) a group whose FIRST frame lies in the padding holds nothing but the clamp value: it is not written at all -- k_logmel_norm and the fetch
      // know the value (two thirds of the 30 s window of a 10 s clip: 163 of the 245 MB this kernel wrote per C3 step, and as many bytes the next pass read back)
      if (!scan && (f_begin + gi * LM_G) * W_HOP - W_NFFT / 2 < len) {
          const int64_t f0 = gi * LM_G;
          const int nj = (int)min<int64_t>(LM_G, n_fr - f0);
          for (int idx = lane; idx < n_mels * LM_G; idx += 64) {
              const int b = idx / LM_G, j = idx - b * LM_G;
              if (j < nj) logspec[((int64_t)clip * n_mels + b) * W_FRAMES + f0 + j] = ob[b * (LM_G + 1) + j];
          }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    }
    vmax = wave_xor_max(vmax);
    if (lane == 0) atomicMax(clip_max + clip, f32_order_key(vmax));
}

// max(x, max - 8), (x + 4) / 4 of clips clip0 .. clip0 + gridDim.z - 1 from the raw log10 values k_logmel_frames left ([clip][n_mels][3000]; frames of the padding
// are not stored: their value is the clamp constant) into what the CALLER consumes: out_tm = the op_t time-major padded image [clip][3002][n_mels] the conv stem
// reads (rows 0 and 3001 stay zero) -- pce_logmel_run; out_f32 = the float matrix [n_mels][3000] of ONE clip in a staging buffer -- pce_logmel_fetch.
// Round 5 rewrote the whole float matrix in place on every run (read 245 MB, write 245 + 123 MB per C3 step: 3.2 x the stage's algorithmic bytes); nothing on the
// device reads it.
__global__ __launch_bounds__(256) void k_logmel_norm(const float *__restrict__ logspec, const unsigned int *__restrict__ clip_max, int n_mels,
                                                    const int64_t *__restrict__ clip_off, const int64_t *__restrict__ frame0, int clip0,
                                                    op_t *__restrict__ out_tm, float *__restrict__ out_f32,
                                                    int2 *__restrict__ skip_c1, int2 *__restrict__ skip_c2)
{
    __shared__ float tile[64][65];
    const int clip = clip0 + blockIdx.z, f0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
    const float floor_v = f32_from_key(clip_max[clip]) - 8.0f;
    const int64_t full = clip_off[clip + 1] - clip_off[clip];
    const int64_t len = frame0 ? full : min<int64_t>(full, (int64_t)W_SAMPLES), f_begin = frame0 ? frame0[clip] : 0;
    if (skip_c1 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        // the row tiles the conv stem leaves out for this clip (ST_TILE above), from the image this launch writes
        const int s = stem_first_skipped_tile(len, f_begin);
        skip_c2[clip] = make_int2(s, ST_C2_LAST - 1);
        skip_c1[clip] = s < ST_C2_LAST ? make_int2(2 * s, ST_C1_KEEP - 1) : make_int2(1, 0);      // conv2 tiles [0, s) read conv1 rows < 2 ST_TILE s
    }
    const float pad_v = (fmaxf(log10f(fmaxf(0.f, 1e-10f)), floor_v) + 4.0f) / 4.0f;           // a frame of the zero padding (k_logmel_frames' own expression)
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const bool padded = (f_begin + f0 + tx) * W_HOP - W_NFFT / 2 >= len;
    for (int r = ty; r < 64; r += 4) {
        const int b = b0 + r, f = f0 + tx;
        if (b < n_mels && f < W_FRAMES) {
            const float v = padded ? pad_v : (fmaxf(logspec[((int64_t)clip * n_mels + b) * W_FRAMES + f], floor_v) + 4.0f) / 4.0f;
            if (out_f32) out_f32[(int64_t)b * W_FRAMES + f] = v;
            tile[r][tx] = v;
        }
    }
    if (!out_tm) return;
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int f = f0 + r, b = b0 + tx;
        if (b < n_mels && f < W_FRAMES) out_tm[((int64_t)clip * (W_FRAMES + 2) + f + 1) * n_mels + b] = (op_t)tile[tx][r];
    }
}
