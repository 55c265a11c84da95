"""tests/frontend_restatement.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

float64 numpy restatements of the two fp32 front ends of the device library, written from the semantics include/pce.h documents and from nothing
else of the project: no torch, none of the oracles' STFTs.  An exact periodic Hann window, numpy.fft.rfft in float64, and the Slaney filter bank of
oracle/whisper_oracle.py (``mel_filters``) taken as given data.  Pinned to the oracles by tests/test_frontend_host.py; the device kernels are held to
it by tests/test_gpu_frontend.py, whose docstring derives the error model that ``logmel_bound`` / ``stft_bound`` below evaluate.

Log-mel (pce_logmel_run / pce_logmel_run_at; whisper.log_mel_spectrogram):
  frame f is centred on sample 160 f: samples 160 f - 200 .. 160 f + 199, reflected at sample 0 (index -i reads sample i), zero past the audio;
  power of the 400-point transform's bins 0 .. 200, mel bands, log10(max(., 1e-10)), max(., M - 8), (. + 4) / 4.
  * pad-or-trim form (``log_mel``): the clip trimmed to 30 s and followed by zeros, frames 0 .. 2999, M = the maximum over those 3000 frames;
  * whole-recording form (``log_mel_window``): every sample of the recording followed by 30 s of zeros, frames start .. start + 2999, M = the maximum
    over every frame that sees audio (and the frames of the window: a frame of pure padding sits at log10(1e-10), the smallest value there is).
STFT in dB (pce_stft_db_run; librosa.amplitude_to_db(abs(librosa.stft(y, 1024, hop)), ref=np.max)):
  1 + len // hop frames centred on sample hop f, zeros on both sides, periodic Hann(1024), bins 0 .. 512;
  10 log10(max(1e-10, |X|^2)) - 10 log10(max(1e-10, ref^2)), ref = the clip's largest |X|, floored at -80.
The two 1e-10 are the float32 nearest to 1e-10 (torch clamps a float32 tensor, librosa's amin^2 meets float32 power): that IS the constant of both
references, 1.3e-8 above the decimal.
"""
import numpy as np

from oracle import whisper_oracle as WO

U = 2.0 ** -24
CLAMP = float(np.float32(1e-10))
N_FFT, HOP, N_SAMPLES, N_FRAMES, N_BINS = 400, 160, 480000, 3000, 201
S_FFT, S_BINS = 1024, 513
TINY = 1e-30                                  # absolute slack for values flushed below the smallest normal number (1e-38 each, a few hundred per sum)


def hann(n):
    """The periodic Hann window, exact in float64."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def gamma(n):
    """n successive roundings: (1 + U)^n - 1 <= n U / (1 - n U)."""
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


class LogMel:
    """out [n_mels][3000]: the result.  Over ALL T frames the clip maximum is taken from (window = frames start .. start + 2999 of them):
    raw [n_mels][T] log10(max(E, 1e-10)), E [n_mels][T] band energies, absX [201][T] |X_k|, S [T] sum_n |x_n w_n|, peak = the maximum of raw."""


def _log_mel_frames(audio, T, n_mels):
    """Frames 0 .. T - 1 of ``audio`` (float64, already trimmed) followed by zeros."""
    r = LogMel()
    n = len(audio)
    Ta = min(T, (n + N_FFT // 2) // HOP + 1)                         # frames Ta .. see zeros alone: transformed as zeros, not one by one
    right = max(0, (Ta - 1) * HOP + N_FFT // 2 - n)
    left = np.zeros(N_FFT // 2)
    m = min(N_FFT // 2, n - 1) if n else 0
    if m > 0:
        left[N_FFT // 2 - m:] = audio[m:0:-1]                        # index -i reads sample i, where sample i exists
    x = np.concatenate([left, audio, np.zeros(right + 1)])
    idx = (np.arange(Ta) * HOP)[:, None] + np.arange(N_FFT)[None, :]
    fr = x[idx] * hann(N_FFT)[None, :]
    r.S = np.zeros(T); r.absX = np.zeros((N_BINS, T))
    r.S[:Ta] = np.abs(fr).sum(axis=1)
    r.absX[:, :Ta] = np.abs(np.fft.rfft(fr, axis=1)).T               # [201][T]
    r.filters = WO.mel_filters(n_mels).astype(np.float64)
    r.E = r.filters @ (r.absX ** 2)
    r.raw = np.log10(np.maximum(r.E, CLAMP))
    r.peak = float(r.raw.max())
    r.n_mels = n_mels
    return r


def _finish(r, start):
    r.start = start
    r.out = (np.maximum(r.raw[:, start:start + N_FRAMES], r.peak - 8.0) + 4.0) / 4.0
    return r


def log_mel(pcm_i16, n_mels=80):
    """Pad-or-trim form: what pce_logmel_run + pce_logmel_fetch document."""
    audio = np.asarray(pcm_i16, dtype=np.float64)[:N_SAMPLES] / 32768.0
    return _finish(_log_mel_frames(audio, N_FRAMES, n_mels), 0)


def log_mel_window(pcm_i16, start_frame, n_mels=80):
    """Whole-recording form: what pce_logmel_run_at + pce_logmel_fetch document."""
    audio = np.asarray(pcm_i16, dtype=np.float64) / 32768.0
    n_audio = (len(audio) + N_FFT // 2) // HOP + 1                   # frames 0 .. n_audio - 1 can see a sample
    return _finish(_log_mel_frames(audio, max(n_audio, start_frame + N_FRAMES), n_mels), int(start_frame))


def _log10_interval(v, dv, clamp):
    """How far log10(max(., clamp)) can move when its argument moves by at most dv from v (the clamp is 1-Lipschitz, the logarithm monotone)."""
    mid = np.log10(np.maximum(v, clamp))
    return np.maximum(np.log10(np.maximum(v + dv, clamp)) - mid, mid - np.log10(np.maximum(v - dv, clamp)))


def _peak_error(value, bound):
    """The error of a computed maximum: the largest bound among the elements that can be the computed maximum at all."""
    if value.size == 0:
        return 0.0
    i = np.unravel_index(np.argmax(value), value.shape)
    cand = value + bound >= value[i] - bound[i]
    return float(bound[cand].max())


def logmel_raw_bound(r, L, eps_log10):
    """Bound on the device's raw log10 values, all T frames (model: tests/test_gpu_frontend.py)."""
    dX = gamma(L) * r.S[None, :]
    dP = 2.0 * r.absX * dX + dX ** 2 + gamma(3) * (r.absX + dX) ** 2
    cnt = (r.filters > 0).sum(axis=1).astype(np.float64)[:, None]
    EdP = r.filters @ dP
    dE = EdP + gamma(cnt + 2) * (r.E + EdP) + 1e-15 * (r.absX ** 2 + dP).sum(axis=0)[None, :] + TINY
    d = _log10_interval(r.E, dE, CLAMP)
    return d + eps_log10 * (np.abs(r.raw) + d)


def logmel_bound(r, L, eps_log10):
    """Bound on |device - r.out| per element [n_mels][3000], and the mask of r's elements above the max - 8 floor."""
    b_raw = logmel_raw_bound(r, L, eps_log10)
    d_peak = _peak_error(r.raw, b_raw)
    d_floor = d_peak + U * (abs(r.peak) + 8.0 + d_peak)              # max - 8.0f rounds once
    w = slice(r.start, r.start + N_FRAMES)
    b = (b_raw[:, w] + d_floor) / 4.0
    b = b + U * (np.abs(r.out) + b)                                  # (x + 4.0f) rounds once, the quarter is exact
    return b, r.raw[:, w] > r.peak - 8.0


class StftDb:
    """out [513][1 + len // hop]; absX |X| [513][frames]; S [frames]; raw = 10 log10(max(1e-10, |X|^2)); ref = max |X|; ref_db."""


def stft_db(pcm_i16, hop):
    r = StftDb()
    a = np.asarray(pcm_i16, dtype=np.float64) / 32768.0
    nf = 1 + len(a) // hop
    x = np.concatenate([np.zeros(S_FFT // 2), a, np.zeros(S_FFT // 2 + hop)])
    w = hann(S_FFT)
    r.absX = np.empty((S_BINS, nf)); r.S = np.empty(nf)
    for f0 in range(0, nf, 2048):                                    # in slabs: hop 1 makes a frame per sample
        f1 = min(nf, f0 + 2048)
        idx = (np.arange(f0, f1) * hop)[:, None] + np.arange(S_FFT)[None, :]
        fr = x[idx] * w[None, :]
        r.S[f0:f1] = np.abs(fr).sum(axis=1)
        r.absX[:, f0:f1] = np.abs(np.fft.rfft(fr, axis=1)).T
    r.raw = 10.0 * np.log10(np.maximum(CLAMP, r.absX ** 2))
    r.ref = float(r.absX.max())
    r.ref_db = 10.0 * np.log10(max(CLAMP, r.ref ** 2))
    r.out = np.maximum(r.raw - r.ref_db, -80.0)
    return r


def stft_bound(r, L, eps_log10):
    """Bound on |device - r.out| per element [513][frames], and the mask of r's elements above -80 dB."""
    dX = gamma(L) * r.S[None, :]
    dmag = dX + gamma(3) * (r.absX + dX)                             # x x + y y: relative 2 U on the square, U after the root, whose own error is one ulp = 2 U
    dP = 2.0 * r.absX * dmag + dmag ** 2 + U * (r.absX + dmag) ** 2  # mag * mag
    P = r.absX ** 2
    d = _log10_interval(P, dP, CLAMP)
    b_raw = 10.0 * (d + eps_log10 * (np.abs(r.raw) / 10.0 + d))
    b_raw = b_raw + U * (np.abs(r.raw) + b_raw)                      # 10.0f * . rounds once
    d_ref = _peak_error(r.absX, dmag)
    R2 = r.ref ** 2
    dR2 = 2.0 * r.ref * d_ref + d_ref ** 2 + U * (r.ref + d_ref) ** 2
    d = float(_log10_interval(np.float64(R2), np.float64(dR2), CLAMP))
    b_ref = 10.0 * (d + eps_log10 * (abs(r.ref_db) / 10.0 + d))
    b_ref = b_ref + U * (abs(r.ref_db) + b_ref)
    b = b_raw + b_ref
    b = b + U * (np.abs(r.raw) + abs(r.ref_db) + b)                  # db - ref_db rounds once; the floor is 1-Lipschitz
    return b, r.raw - r.ref_db > -80.0
