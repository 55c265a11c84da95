"""The two hand-written fp32 transforms that turn PCM into everything downstream -- the log-mel front end of the Whisper leg (k_logmel_frames,
k_logmel_norm: the fetched fp32 matrix AND, through pce_selftest_logmel_image, the 16-bit time-major image the encoder reads) and the STFT in dB
(k_stft_raw + k_stft_norm on fetch, k_stft_norm in place, k_stft_max + k_stft_db) -- against the float64 restatement tests/frontend_restatement.py
(pinned to the oracles by tests/test_frontend_host.py), at every edge of their frame, padding, store-group and alignment logic.  Every element of
every output is compared, none excused, against a bound DERIVED from the kernels' rounding counts, not fitted.  U = 2^-24.

Transform.  Every computed bin is  sum_n x_n w_n omega^(nk) (1 + theta_n),  |theta_n| <= L U  (first order; the bound functions use n U / (1 - n U)),
hence |dX_k| <= L U S,  S = sum_n |x_n w_n|.  L counts the roundings on one input's path to one output; a complex product formed as
(a.x w.x - a.y w.y, a.x w.y + a.y w.x) with r roundings per component moves the VECTOR by at most sqrt(2) r U |a| |w| (Cauchy-Schwarz on each component,
tight), a complex sum or a real-times-complex product by r U of its own modulus.  (int16 -> float and the 2^-15 scale are exact.)
  Log-mel (k_logmel_frames; the disassembly holds v_fmac for stage A only, separate v_mul / v_sub / v_add elsewhere: nothing is contracted):
      window      table rounded from double 1, x * w 1                                                   2
      stage A     w16 table 1, 16 fmaf into the accumulator (x real: no sqrt 2)                         17
      twiddle     w400 table 1, mul + sub|add per component 2 sqrt(2)                                    3.83
      stage B     w25 table 1, product 2 sqrt(2), 25 additions into the accumulator                     28.83     (sum |Y| <= S)
      L_LOGMEL = 52   (51.66)
  STFT (stft_frame; inline-asm packed mul / add, no fma), 1024 reals as 512 complex z_n, |z_n| <= |x_2n w_2n| + |x_2n+1 w_2n+1|:
      window      table 1, x * w 1                                                                       2
      dft8 x 3    longest path a -> b (1) -> add_mi (1) -> * h (1, h rounded 1) -> d1 (1) -> out (1)      18
      twiddles    passes 2 and 3: table 1 + 2 sqrt(2) each                                               7.66        L_Z = 27.66
      untangle    X_k = (1 + T)/2 Z_k + (1 - T)/2 conj Z_(M-k), |T| = 1: the two moduli a, b have a^2 + b^2 = 1, a + b <= sqrt 2:  sqrt(2) L_Z = 39.1;
                  its own roundings act on moduli <= S: e 1, o 1 + (table 1 + 2 sqrt 2), the last addition 1                  6.83
      L_STFT = 46   (45.95)
Power.  dP <= 2 |X| dX + dX^2 + own roundings: log-mel re re + im im, 3 U (P + dP); STFT sqrt(x x + y y) (2 U on the square, U after the root, 2 U = one
ulp for v_sqrt_f32) then mag mag (U).  Mel band: dE_b <= sum_k w_bk dP_k + (cnt_b + 2) U E_b -- cnt_b fmaf of positive terms, and the library's own
table of the same filters (double, rounded once) against WO.mel_filters (double, rounded once): one ulp = 2 U apart at most (+ 1e-15 of the frame's power
for weights that cancel at a band's edge).
Logarithm.  log10(max(., 1e-10)) is monotone behind a 1-Lipschitz clamp: the argument's interval maps to the value's interval exactly; the device
logarithm adds EPS_LOG10 |log10|.  STFT: 10 * . rounds once, for the element and for ref_db = 10 log10(max(1e-10, ref^2)); db - ref_db rounds once.
Clamp and scale.  max - 8 (one rounding) and the -80 floor are 1-Lipschitz: an element's bound is its own plus the clip maximum's, which is the largest
bound among the elements that lie within their bounds of the maximum; log-mel then (x + 4) / 4, one rounding.  No allowance near a floor.

EPS_LOG10.  Neither the headers nor the documents installed with the compiler state an accuracy for the device's log10f (__log10f and log10f are both
__builtin_log10f in this toolchain's __clang_hip_math.h, the library is built without fast-math: ONE function for the three call sites).  It is probed
(test_log_probe, asserted on every run) on arguments known independently of the transform's data path: unit impulses of amplitude 2^0 .. 2^15 at a
frame's centre meet the window's tap 1, and since every other input is an exact zero the log-mel transform returns |X_k| = A / 32768 EXACTLY (stage A
multiplies by w16[0] = 1 or w16[8] = -1, the twiddle and stage B by their entries 0 = 1; sums with zeros are exact); a band's energy is then
A^2 2^-30 sum_k w_bk up to the cnt_b + 2 roundings above, and the fetched value gives the raw logarithm back up to U |raw + 4|.  Bands of at most three
bins, and the all-zero clip (argument exactly the clamp), are read: resolution ((cnt_b + 2) U / ln 10 + U |raw + 4|) / |raw| <= 3 U.
EPS_LOG10 = 4 x max(measured, resolution, 2^-23); the 4 x is the project's margin for arguments a probe does not see.
The STFT cannot resolve as finely: its twiddle products leave up to L_STFT U on |X| and on the reference even for an impulse.  Its probe (hop 1024, an
impulse of 2^j at the centre of frame j, the loudest frame as the reference; two clips, topped by 2^15 and by 2^8, so that every amplitude is read
above the -80 dB floor and at least 18 dB below the reference) is asserted to lie within that resolution + EPS_LOG10 / 4 for each of its two logarithms.
Measured on an MI355X, fp16 and bf16 build, 80 and 128 mels alike: worst |raw - want| / |want| = 1.933e-7 = 3.24 U (EPS_LOG10_MEASURED) against a
resolution of 2.94 U (asserted <= 3 U = 1.788e-7) and the floor 2^-23 = 1.192e-7:  EPS_LOG10 = 4 x 1.933e-7 = 7.732e-7.  The STFT probe deviates by
2.49e-7 = 4.18 U relative at worst, far inside its own resolution (up to 51 U).

Worst |got - want| / bound per case family on an MI355X with these constants.  The fp16 and the bf16 build agree in every digit (the kernels hold no
16-bit operand before the image's final cast), and no ratio came near 1: no miscount and no bug was found.
    log-mel                          80 mels    128 mels          STFT, every form bit-identical      lengths    content
    lengths 0 .. 1001                  0.057       0.057          hop 256                               0.059      0.089
    store groups, P = 16 .. 32         0.021       0.019          hop 255                               0.066      0.091
    content                            0.057       0.057          hop 1                                 0.085      0.079
    479 999 .. 496 000 samples         0.016       0.018          hop 1000                              0.050      0.089
    windows (pce_logmel_run_at)        0.027       0.027          hop 1024                              0.050      0.089
    image sequences (fetch)            0.029 (80 and 128 mels, all three operand modes; image = rounded fetch bit for bit in every step)
The ratios sit well below 1 because the bound is a worst case over the signs of up to 52 (46) roundings per path while the errors of a transform add
up like a random walk; what the bound buys is in tests/test_frontend_host.py: on flat spectra it is ten (four) times under what the suite asked before.
"""
import ctypes as C
import os

import numpy as np
import pytest

import prosody_control_french_tts_amd as pkg
from prosody_control_french_tts_amd import PceError
from oracle import whisper_oracle as WO
from tests import frontend_cases as FC
from tests import frontend_restatement as R

U = 2.0 ** -24
L_LOGMEL = 52
L_STFT = 46
EPS_LOG10_MEASURED = 1.933e-7                 # test_log_probe on an MI355X, both builds, 80 and 128 mels (see the docstring)
EPS_LOG10_RESOLUTION = 3 * U
EPS_LOG10 = 4 * max(EPS_LOG10_MEASURED, EPS_LOG10_RESOLUTION, 2.0 ** -23)
BUILDS = ("fp16", "bf16")
HOPS = (256, 255, 1, 1000, 1024)


# ---------------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ref_logmel(pcm, n_mels, start=None):
    r = R.log_mel(pcm, n_mels) if start is None else R.log_mel_window(pcm, start, n_mels)
    b, _ = R.logmel_bound(r, L_LOGMEL, EPS_LOG10)
    return r.out, b


def _check_logmel(engine, clips, n_mels, starts, refs, family):
    """Upload, run in both builds, compare every element of every clip; -> the worst ratio per build."""
    engine.upload(clips, 16000)
    worst = {}
    for build in BUILDS:
        engine.whisper_set_operands(build)
        if starts is None:
            engine.logmel_run(n_mels)
        else:
            engine.logmel_run_at(n_mels, starts)
        w = 0.0
        for i, (want, bound) in enumerate(refs):
            got = engine.logmel_fetch(i)
            assert got.shape == (n_mels, 3000) and got.dtype == np.float32 and np.isfinite(got).all()
            ratio = np.abs(got.astype(np.float64) - want) / bound
            k = np.unravel_index(np.argmax(ratio), ratio.shape)
            w = max(w, float(ratio[k]))
            assert ratio[k] <= 1.0, (family, build, n_mels, i, len(clips[i]), None if starts is None else starts[i], k, float(got[k]), float(want[k]), float(bound[k]))
        worst[build] = w
    print(f"log-mel {family} {n_mels} mels: worst |got - want| / bound " + ", ".join(f"{b} {worst[b]:.3f}" for b in BUILDS))
    return worst


def _to_bits(x32, build):
    """float32 -> the 16-bit operand type, round to nearest even, as bit patterns."""
    if build.startswith("fp16"):
        return x32.astype(np.float16).view(np.uint16)
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@pytest.fixture(scope="module")
def two_fft():
    """A second context with the two-FFT switch (k_stft_max + k_stft_db), created as tests/test_gpu_edges.py creates it."""
    old = os.environ.get("PCE_STFT_TWO_FFT")
    os.environ["PCE_STFT_TWO_FFT"] = "1"
    try:
        eng = pkg.ProsodyEngine(0)
    finally:
        if old is None:
            os.environ.pop("PCE_STFT_TWO_FFT", None)
        else:
            os.environ["PCE_STFT_TWO_FFT"] = old
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the logarithm probe
# ---------------------------------------------------------------------------------------------------------------------------------------
def _amp(j):
    return -32768 if j == 15 else 1 << j


@pytest.mark.gpu
def test_log_probe(engine):
    """The device's log10f on arguments known without the transform (see the docstring): measured relative error, the probe's resolution, the constant."""
    # log-mel: three clips so that no impulse falls under another's max - 8; frame centres three frames apart (480 samples: frames do not share an impulse)
    groups = [list(range(0, 6)), list(range(6, 11)), list(range(11, 16))]
    clips = [FC.impulses(480 * len(g) + 400, [480 * (q + 1) for q in range(len(g))], [_amp(j) for j in g]) for g in groups] + [FC.silence(1000)]
    engine.upload(clips, 16000)
    measured, resolution = 0.0, 0.0
    for build in BUILDS:
        engine.whisper_set_operands(build)
        for n_mels in (80, 128):
            filt = WO.mel_filters(n_mels).astype(np.float64)
            cnt = (filt > 0).sum(axis=1)
            bands = np.nonzero(cnt <= 3)[0]
            assert len(bands) >= 40
            engine.logmel_run(n_mels)
            for ci, g in enumerate(groups + [[]]):
                got = engine.logmel_fetch(ci).astype(np.float64)
                peak = max([np.log10(np.maximum(filt.sum(axis=1) * (abs(_amp(j)) / 32768.0) ** 2, R.CLAMP)).max() for j in g] + [np.log10(R.CLAMP)])
                cases = [(3 * (q + 1), (abs(_amp(j)) / 32768.0) ** 2) for q, j in enumerate(g)]               # (frame, |X|^2)
                if np.log10(R.CLAMP) > peak - 8.0 + 1e-3:
                    cases.append((2999, 0.0))                                                                # a frame of the padding: the argument is the clamp itself
                for frame, p in cases:
                    want = np.log10(np.maximum(filt[bands].sum(axis=1) * p, R.CLAMP))
                    assert (want > peak - 8.0 + 1e-3).all()                                                  # no probe value is clamped by the maximum
                    raw = 4.0 * got[bands, frame] - 4.0
                    measured = max(measured, float(np.max(np.abs(raw - want) / np.abs(want))))
                    resolution = max(resolution, float(np.max(((cnt[bands] + 2) * U / np.log(10.0) + U * np.abs(want + 4.0)) / np.abs(want))))
    print(f"log10f probe (log-mel): measured {measured:.3e} = {measured / U:.2f} U, resolution {resolution:.3e} = {resolution / U:.2f} U, "
          f"EPS_LOG10 = {EPS_LOG10:.3e}")
    assert resolution <= EPS_LOG10_RESOLUTION
    assert measured <= EPS_LOG10
    # STFT: hop 1024, frame j sees the impulse 2^j at its centre 1024 j alone and the loudest frame is the reference:  want = 20 (j - top) log10 2.  Two clips,
    # top = 15 and top = 8, so that every amplitude is read above the -80 dB floor; |want| >= 18 dB: nearer to the reference the RELATIVE error of a value
    # near zero measures nothing
    clips = [FC.impulses(1024 * (top + 1) + 1, [1024 * j for j in range(top + 1)], [_amp(j) for j in range(top + 1)]) for top in (15, 8)]
    engine.upload(clips, 16000)
    engine.stft_db_run(1024, 1024)
    worst, res_rel = 0.0, 0.0
    for ci, top in enumerate((15, 8)):
        got = engine.stft_db_fetch(ci).astype(np.float64)
        assert got.shape == (513, top + 2)
        for j in range(max(0, top - 13), top - 2):
            want = 20.0 * (j - top) * np.log10(2.0)
            res = 2 * 10.0 * (2 * L_STFT + 8) * U / np.log(10.0) + 3 * U * abs(want)   # |X| and ref within L_STFT U each, the power's own roundings; 10 * . twice, the difference
            err = np.abs(got[:, j] - want)
            worst = max(worst, float(np.max(err / abs(want))))
            res_rel = max(res_rel, res / abs(want))
            assert (err <= res + 2 * EPS_LOG10 / 4 * 10.0 * np.log10(2.0 ** 30)).all(), (top, j, float(err.max()), res)      # two logarithms, each of an argument >= 2^-30
    print(f"log10f probe (STFT): worst relative deviation {worst:.3e} = {worst / U:.2f} U (resolution of this probe: up to {res_rel / U:.1f} U)")


# ---------------------------------------------------------------------------------------------------------------------------------------
# log-mel: lengths, content, windows
# ---------------------------------------------------------------------------------------------------------------------------------------
F_EDGE = 5                                                         # 160 f + 200 + r: the first padded frame moves from f + 3 to f + 4 between r = 0 and r = 1
SHORT_LENGTHS = (0, 1, 199, 200, 201, 359, 360, 361, 160 * F_EDGE + 199, 160 * F_EDGE + 200, 160 * F_EDGE + 201)
# the first padded frame P = ceil((len + 200) / 160) at every residue of the 16-frame store group: len = 160 P - 200, P = 16 .. 32.  P = 17: group 16 .. 31
# holds audio in its first frame alone; P = 31 / 32: fifteen frames of audio and one of padding / a full group followed by one that is not written at all
GROUP_LENGTHS = tuple(160 * P - 200 for P in range(16, 33))


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_short_lengths(engine, n_mels):
    clips = [FC.content(FC.CONTENTS[1 + i % 6], n, seed=i) for i, n in enumerate(SHORT_LENGTHS)]
    _check_logmel(engine, clips, n_mels, None, [_ref_logmel(c, n_mels) for c in clips], "lengths 0 .. 1001")
    for part, name in ((GROUP_LENGTHS[:9], "store groups, P = 16 .. 24"), (GROUP_LENGTHS[9:], "store groups, P = 25 .. 32")):
        clips = [FC.noise(n, 40 + i, 2000.0) for i, n in enumerate(part)]
        for c in clips:
            P = -(-(len(c) + 200) // 160)
            assert P * 160 - 200 >= len(c) > (P - 1) * 160 - 200
        _check_logmel(engine, clips, n_mels, None, [_ref_logmel(c, n_mels) for c in clips], name)


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_content(engine, n_mels):
    n = FC.FLAT_N
    clips = [x for _, x in FC.flat_inputs()] + [FC.silence(n), FC.square(n + 1), FC.dc_min(n - 1), FC.tone(n + 3), FC.loud_then_lsb(2 * n + 5)]
    clips += [FC.impulses(3000, p, a) for p, a in ((0, 1), (1, 1), (199, 1), (200, 1), (160 * 7, 1))]
    assert len(clips) <= 12
    refs = [_ref_logmel(c, n_mels) for c in clips]
    lsb = R.log_mel(clips[1], n_mels)
    assert lsb.raw.max() < 0                                                           # the order key of the maximum sees negative floats only
    loud = R.log_mel(clips[6], n_mels)
    assert (loud.raw[:, 40:200] < loud.peak - 8.0).mean() > 0.9                        # the max - 8 clamp bites in the quiet part
    _check_logmel(engine, clips, n_mels, None, refs, "content")


def _long_clips():
    quiet = FC.noise(496000, 50, 300.0)
    quiet[480000:] = FC.noise(16000, 51, 9000.0)                                        # 31 s: the last second is 30 dB louder
    base = FC.noise(480001, 52, 3000.0)
    return [base[:479999], base[:480000], base, quiet]


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_30s_lengths(engine, n_mels):
    clips = _long_clips()
    refs = [_ref_logmel(c, n_mels) for c in clips]
    assert np.array_equal(refs[3][0], R.log_mel(clips[3][:480000], n_mels).out)         # pce_logmel_run ignores what lies beyond 30 s
    _check_logmel(engine, clips, n_mels, None, refs, "479 999 .. 496 000 samples")


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_windows(engine, n_mels):
    a = FC.noise(24037, 60, 3000.0)
    burst_first = FC.loud_then_lsb(32000, seed=61)
    long_clip = _long_clips()[3]
    clips = [a] * 6 + [burst_first, long_clip, long_clip, FC.tone(501)]
    starts = [0, 1, 15, 16, 17, len(a) // 160, 100, 0, 100, 3]
    refs = [_ref_logmel(c, n_mels, s) for c, s in zip(clips, starts)]
    w_quiet = R.log_mel_window(burst_first, 100, n_mels)
    assert w_quiet.raw[:, :100].max() == w_quiet.peak and w_quiet.raw[:, 100:].max() < w_quiet.peak - 8.0      # the clamp comes from a burst BEFORE the window
    w_long = R.log_mel_window(long_clip, 0, n_mels)
    assert w_long.raw[:, 3000:].max() == w_long.peak > w_long.raw[:, :3000].max() + 2.0                          # ... and from one BEHIND it
    assert not np.array_equal(refs[7][0], R.log_mel(long_clip, n_mels).out)             # pce_logmel_run_at sees what lies beyond 30 s
    _check_logmel(engine, clips, n_mels, starts, refs, "windows")
    with pytest.raises(PceError):
        engine.logmel_run_at(n_mels, [0] * 9 + [4])                                     # 4 * 160 > 501 samples


# ---------------------------------------------------------------------------------------------------------------------------------------
# the 16-bit time-major image
# ---------------------------------------------------------------------------------------------------------------------------------------
def _check_image(engine, build, clips, n_mels, starts, step, memo):
    worst = 0.0
    for i, c in enumerate(clips):
        got = engine.logmel_fetch(i)
        img = engine.selftest_logmel_image(i)
        assert img.shape == (3002, n_mels) and img.dtype == np.uint16
        assert not img[0].any() and not img[3001].any(), (step, i)
        assert np.array_equal(img[1:3001], _to_bits(np.ascontiguousarray(got.T), build)), (step, i)
        key = (id(c), n_mels, None if starts is None else starts[i])
        if key not in memo:
            memo[key] = _ref_logmel(c, *key[1:])
        want, bound = memo[key]
        worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - want) / bound)))
        assert worst <= 1.0, (step, i)
        # a padded frame holds THIS run's pad value: (max(log10(1e-10), max - 8) + 4) / 4 of the restatement, to the bound, in every band, in the image too
        P = -(-(len(c) + 200) // 160) - (0 if starts is None else starts[i])
        if 0 <= P < 3000:
            assert np.array_equal(img[3000], _to_bits(got[:, 2999], build)) and (np.abs(got[:, P:] - want[:, P:]) <= bound[:, P:]).all()
            assert (img[P + 1:3001] == img[3000][None, :]).all(), (step, i)
    return worst


@pytest.mark.gpu
def test_logmel_image(engine, ops):
    """What the encoder reads: rows 1 .. 3000 of the image are the fetched fp32 matrix, transposed and rounded to the operand type, bit for bit; rows 0
    and 3001 are zero -- also after the sequences that could leave stale data behind (the zero rows are memset only when the buffer's capacity or
    n_mels changes; padded groups of frames are never written to the fp32 buffer)."""
    build = ops["name"]
    big = FC.noise(480000, 70, 8000.0)
    shorts = [FC.lsb_noise(16000, 71), FC.noise(4801, 72, 500.0)]
    five = [FC.noise(n, 73 + i, 1000.0 * (i + 1)) for i, n in enumerate((2360, 7001, 160, 12345, 5000))]
    worst, memo = 0.0, {}
    engine.upload([big] * 5, 16000); engine.logmel_run(128)
    worst = max(worst, _check_image(engine, build, [big] * 5, 128, None, "loud 30 s batch", memo))
    engine.upload(shorts, 16000)
    for step, nm in enumerate((128, 80, 128)):
        engine.logmel_run(nm)
        worst = max(worst, _check_image(engine, build, shorts, nm, None, f"short batch after the loud one, {nm} mels (step {step})", memo))
    for step, batch in enumerate((five, shorts, five)):
        engine.upload(batch, 16000); engine.logmel_run(80)
        worst = max(worst, _check_image(engine, build, batch, 80, None, f"5 clips, 2, 5 (step {step})", memo))
    starts = [3, 0, 1, 16, 31]
    engine.logmel_run_at(80, starts)
    worst = max(worst, _check_image(engine, build, five, 80, starts, "run_at", memo))
    engine.logmel_run(80)
    worst = max(worst, _check_image(engine, build, five, 80, None, "run after run_at", memo))
    print(f"log-mel image {build}: bit-identical to the rounded fetch in every step; worst |fetch - want| / bound {worst:.3f}")


@pytest.mark.gpu
def test_logmel_image_hook_refusals(engine):
    with pkg.ProsodyEngine(0) as fresh:
        fresh.upload([FC.noise(1000, 80)], 16000)
        for build in BUILDS:
            fresh.whisper_set_operands(build)
            with pytest.raises(PceError, match="status -4"):                            # PCE_E_STATE: before a run of this operand build
                fresh.selftest_logmel_image(0)
            fresh.logmel_run(80)
            assert fresh.selftest_logmel_image(0).shape == (3002, 80)
            for clip in (-1, 1):
                with pytest.raises(PceError, match="status -1"):                        # PCE_E_INVALID
                    fresh.selftest_logmel_image(clip)


# ---------------------------------------------------------------------------------------------------------------------------------------
# STFT in dB
# ---------------------------------------------------------------------------------------------------------------------------------------
def _device_matrix(engine):
    ptr, nbytes = engine.stft_db_device()
    host = np.empty(nbytes // 4, dtype=np.float32)
    engine.sync()
    assert C.CDLL("libamdhip64.so").hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(ptr), C.c_size_t(nbytes), 2) == 0        # hipMemcpyDeviceToHost
    return host


def _check_stft(engine, two_fft, clips, hop, family):
    refs = []
    for c in clips:
        r = R.stft_db(c, hop)
        refs.append((r.out, R.stft_bound(r, L_STFT, EPS_LOG10)[0]))
    engine.upload(clips, 16000); engine.stft_db_run(1024, hop)
    two_fft.upload(clips, 16000); two_fft.stft_db_run(1024, hop)
    worst, outs = 0.0, []
    for i, (want, bound) in enumerate(refs):
        got = engine.stft_db_fetch(i)
        assert got.shape == want.shape == (513, 1 + len(clips[i]) // hop) and got.dtype == np.float32
        assert got.max() <= 0.0 and got.min() >= -80.0, (family, hop, i)
        ratio = np.abs(got.astype(np.float64) - want) / bound
        k = np.unravel_index(np.argmax(ratio), ratio.shape)
        worst = max(worst, float(ratio[k]))
        assert ratio[k] <= 1.0, (family, hop, i, len(clips[i]), k, float(got[k]), float(want[k]), float(bound[k]))
        assert two_fft.stft_db_fetch(i).tobytes() == got.tobytes(), (family, hop, i)     # k_stft_max + k_stft_db: the same bits
        outs.append(got)
    flat = _device_matrix(engine)                                                        # k_stft_norm in place: the same bits, and fetches read them as they are
    assert flat.tobytes() == b"".join(o.tobytes() for o in outs), (family, hop)
    for i in (len(clips) - 1, 0):
        assert engine.stft_db_fetch(i).tobytes() == outs[i].tobytes(), (family, hop, i)
    print(f"STFT hop {hop} {family}: worst |got - want| / bound {worst:.3f}; two-FFT form and in-place form bit-identical")
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("hop", HOPS)
def test_stft_db(engine, two_fft, hop):
    k16 = 8 if hop == 1 else 1                                                           # hop * 16 k: the edge of a 16-frame tile
    lengths = [0, 1, 511, 512, 513, 1023, 1024, 1025, hop * 16 * k16 - 1, hop * 16 * k16, hop * 16 * k16 + 1]
    clips = [FC.content(FC.CONTENTS[1 + i % 6], n, seed=i) for i, n in enumerate(lengths)]
    _check_stft(engine, two_fft, clips, hop, "lengths")
    # content; an odd-length clip first and the same content again: the second copy starts at an odd sample offset, where no frame takes the
    # `interior` path of aligned 4-byte loads -- the two copies must agree bit for bit
    n = 1301 if hop == 1 else FC.FLAT_N
    x = FC.noise(n | 1, 90, 3000.0)
    assert len(x) >= 1024 + 2 * hop                                                      # there ARE interior frames for the two copies to differ in
    clips = [x, x, FC.lsb_noise(n, 2), FC.silence(n // 2), FC.square(n + 1), FC.dc_min(n), FC.tone(n + 2), FC.loud_then_lsb(n + 1, loud=n // 4),
             FC.impulses(n, [0, 1, 199, 200, 3 * hop if hop > 1 else 300], [1, 1, 1, 1, 1000]), FC.tone(n | 1), FC.tone(n | 1)]
    offsets = np.cumsum([0] + [len(c) for c in clips])
    assert offsets[1] % 2 == 1 and offsets[0] % 2 == 0 and offsets[9] % 2 != offsets[10] % 2
    outs = _check_stft(engine, two_fft, clips, hop, "content")
    assert outs[0].tobytes() == outs[1].tobytes() and outs[9].tobytes() == outs[10].tobytes()


@pytest.mark.gpu
def test_stft_db_refuses_bad_hops(engine):
    engine.upload([FC.noise(3000, 95)], 16000)
    for hop in (0, 1025, -1):
        with pytest.raises(PceError):
            engine.stft_db_run(1024, hop)
    engine.stft_db_run(1024, 1024)
    assert engine.stft_db_fetch(0).shape == (513, 3)
