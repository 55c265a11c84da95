"""``Code/Pipeline/evaluate_voice.ipynb`` (cells 518367fb / 31c28b52) with the compute on the engine: score a synthesis against the
recording it imitates -- RMSE of log-F0 along a DTW path, F1 of the phrase breaks, word error rate of the transcripts.

Same function names, argument names and defaults as the notebook where they still mean something; every function has a batched form,
and ``evaluate_all`` runs each stage once over all episodes.

What is restated from packages that are absent here (**parity unpinned**: no run of the originals is available to pin against; the
restatements are checked against independent Python restatements in tests/test_evaluate_voice_host.py / tests/test_gpu_evaluate_voice.py):

* ``fastdtw.fastdtw`` (Salvador & Chan; the package's pure-Python ``__fastdtw`` / ``__reduce_by_half`` / ``__expand_window`` / ``__dtw``):
  the halving and the windows are numpy on the host, every level's dynamic programme is one ``ProsodyEngine.dtw_series`` call
  (``pce_dtw_series``: candidates up, left, diagonal compared as sums, the first minimum wins).
* ``jiwer.wer`` with its default transforms (``RemoveMultipleSpaces``, ``Strip``, split on ``" "``): words become integer ids on the host,
  the edit distance is ``pce_levenshtein`` on the id sequences.
* F0: the notebook's TEXT names ``librosa.pyin`` (hop 512), its CODE calls torchcrepe (``extract_f0_torchcrepe``: ``model="full"``, Viterbi
  decoding, periodicity threshold 0.1).  Both are here.  ``f0="pyin"`` (every default) is the engine's probabilistic YIN (``pce_pyin_*``).
  ``f0="crepe"`` is the notebook's code path on the engine (``pce_crepe_*``): torchcrepe restated from its published implementation and checked
  against a float64 restatement ON RANDOM WEIGHTS (tests/test_gpu_crepe.py) -- no trained checkpoint ships with this project, so the caller
  passes their own ``full.pth`` / ``tiny.pth`` as ``crepe_weights=``; without one ``f0="crepe"`` raises.  Deviations from torchcrepe: audio at
  another rate goes through the engine's ``resample`` (``scipy.signal.resample_poly``'s design; torchcrepe calls resampy), and the random
  one-bin dither of its decoders is not applied.  The RMSE values printed in the notebook are expected only with ``f0="crepe"`` and the
  checkpoint the notebook used, and then only as closely as those two deviations and fp16 operands allow: that has not been measured.
  F1 and WER depend on the Whisper checkpoint only.
* Language: the notebook's ``model.transcribe(path)`` detects it; here it is an argument whose default stays ``"fr"``, and ``language=None``
  detects it per recording as openai-whisper's ``detect_language`` does on the first 30 s window (``Aligners.decoding.detect_language`` ->
  ``pce_whisper_detect_language``; pinned to the ``transformers`` forward by tests/golden/whisper_langid_tiny.npz in tests/test_gpu_langid.py).
* No plotting and no ``compare_episode`` HTML diff.
"""
from __future__ import annotations

import json
import re
import wave
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np

from .. import hostrules as H

C2_HZ = 440.0 * 2.0 ** ((36 - 69) / 12.0)          # librosa.note_to_hz("C2") = 65.406...
C6_HZ = 440.0 * 2.0 ** ((84 - 69) / 12.0)          # librosa.note_to_hz("C6") = 1046.502...
DTW_OK, DTW_EMPTY, DTW_NO_PATH = 0, 1, 2


def _engine(engine):
    if engine is not None:
        return engine
    from ..engine import get_default_engine
    return get_default_engine()


# --------------------------------------------------------------------------------------------------------- fastdtw
def reduce_by_half(x: np.ndarray) -> np.ndarray:
    """``__reduce_by_half``: ``[(x[i] + x[i + 1]) / 2 for i in range(0, len(x) - len(x) % 2, 2)]`` (an odd tail is dropped)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x) - len(x) % 2
    return (x[0:n:2] + x[1:n:2]) / 2


def expand_window(path: np.ndarray, len_x: int, len_y: int, radius: int):
    """``__expand_window``: the coarse ``path`` [k, 2] widened by ``radius`` cells in every direction, projected to the fine grid
    (every coarse cell = 2 x 2 fine cells) and scanned row by row into one contiguous run per row -> ``(lo, hi)`` int32 [len_x], row i
    holding columns ``[lo[i], hi[i])``.  For a monotone path the widened cell set of a fine row i is exactly the union of
    ``[2 (cj - radius), 2 (cj + radius) + 2)`` over the path cells (ci, cj) with ``|ci - i // 2| <= radius``: contiguous, so the
    package's scan keeps all of it, and both ends are non-decreasing in i, so its scan start never skips a run.  A row beyond the
    widened rows (radius 0, odd ``len_x``) is empty (``lo == hi``): the package's own ``__dtw`` then fails with a KeyError."""
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    nc = int(path[-1, 0]) + 1
    cmin = np.full(nc, np.iinfo(np.int64).max); cmax = np.full(nc, -1)
    np.minimum.at(cmin, path[:, 0], path[:, 1]); np.maximum.at(cmax, path[:, 0], path[:, 1])
    c = np.arange(len_x, dtype=np.int64) // 2
    live = c - radius <= nc - 1
    lo = 2 * (cmin[np.clip(c - radius, 0, nc - 1)] - radius)
    hi = 2 * (cmax[np.clip(c + radius, 0, nc - 1)] + radius) + 2
    lo = np.clip(lo, 0, len_y); hi = np.clip(hi, 0, len_y)
    lo = np.where(live, lo, 0); hi = np.where(live, np.maximum(hi, lo), 0)
    return lo.astype(np.int32), hi.astype(np.int32)


def fastdtw_batch(pairs, radius: int = 25, engine=None, dtw_series=None):
    """``fastdtw(x, y, radius)`` of every pair -> [(dist, path int32 [k, 2]), ...].  The recursion of every pair is unrolled into
    its levels (halve until a side is shorter than ``radius + 2``); the coarsest level of every pair runs first, and level by level
    the pairs that still have a finer one run together: one ``dtw_series`` call per level, for all pairs.  ``dtw_series``: a callable
    with the signature of ``ProsodyEngine.dtw_series`` (default: the engine's)."""
    run = dtw_series if dtw_series is not None else _engine(engine).dtw_series
    radius = int(radius)
    if radius < 0:
        radius = 0                                                   # (the package: ``if radius < 0: radius = 0``)
    chains = []
    for x, y in pairs:
        lv = [(np.ascontiguousarray(x, dtype=np.float64).reshape(-1), np.ascontiguousarray(y, dtype=np.float64).reshape(-1))]
        while len(lv[-1][0]) >= radius + 2 and len(lv[-1][1]) >= radius + 2:
            lv.append((reduce_by_half(lv[-1][0]), reduce_by_half(lv[-1][1])))
        chains.append(lv)
    result: List[Optional[tuple]] = [None] * len(chains)
    for h in range(max((len(lv) for lv in chains), default=0)):
        who = [q for q, lv in enumerate(chains) if len(lv) > h]
        batch, wins = [], []
        for q in who:
            x, y = chains[q][len(chains[q]) - 1 - h]
            batch.append((x, y))
            if h == 0:
                wins.append(None)                                    # the coarsest level: the package's exact ``dtw``
            else:
                if not len(result[q][1]):
                    raise ValueError("fastdtw: a level has no path to project")
                wins.append(expand_window(result[q][1], len(x), len(y), radius))
        for q, (path, dist, status) in zip(who, run(batch, wins)):
            if status == DTW_NO_PATH:
                raise ValueError(f"fastdtw(radius={radius}): the projected window admits no path (the package raises KeyError here)")
            result[q] = (dist, path)
    return result


def fastdtw(x, y, radius: int = 25, engine=None, dtw_series=None):
    """``fastdtw.fastdtw(x, y, radius=radius)`` for 1-D series with the package's default distance ``abs(a - b)`` -> ``(dist, path)``;
    ``path`` is an int32 array [k, 2] (the package returns a list of tuples with the same entries).  Restated, parity unpinned."""
    return fastdtw_batch([(x, y)], radius, engine, dtw_series)[0]


# --------------------------------------------------------------------------------------------------------- log-F0 RMSE
def rmse_from_path(log_r: np.ndarray, log_s: np.ndarray, wp: np.ndarray) -> float:
    """The notebook's last two lines: ``sqrt(mean((log_r[wp[:, 0]] - log_s[wp[:, 1]]) ** 2))``."""
    diffs = log_r[wp[:, 0]] - log_s[wp[:, 1]]
    return float(np.sqrt(np.mean(diffs ** 2)))


def f0_contour_rmse_batch(contours, method: str = "fastdtw", radius: int = 25, engine=None, dtw_series=None) -> List[float]:
    """Contour level of ``compute_f0_rmse``: ``contours`` = [(f0_ref, f0_sys), ...], F0 in Hz with NaN where unvoiced -> one RMSE of
    log-F0 per pair (NaN when a side has no voiced frame).  ``method``: ``"fastdtw"`` (the notebook's ``fastdtw(..., radius=25)``) or
    ``"exact"`` (the unwindowed dynamic programme)."""
    if method not in ("fastdtw", "exact"):
        raise ValueError('method: "fastdtw" or "exact"')
    logs, todo = [], []
    for k, (f0_ref, f0_sys) in enumerate(contours):
        f0_ref = np.asarray(f0_ref, dtype=np.float64); f0_sys = np.asarray(f0_sys, dtype=np.float64)
        log_r = np.log(f0_ref[~np.isnan(f0_ref)]); log_s = np.log(f0_sys[~np.isnan(f0_sys)])
        logs.append((log_r, log_s))
        if log_r.size and log_s.size:
            todo.append(k)
    out = [float("nan")] * len(logs)
    if todo:
        batch = [logs[k] for k in todo]
        if method == "fastdtw":
            paths = [p for _, p in fastdtw_batch(batch, radius, engine, dtw_series)]
        else:
            run = dtw_series if dtw_series is not None else _engine(engine).dtw_series
            paths = [p for p, _, _ in run(batch, None)]
        for k, wp in zip(todo, paths):
            out[k] = rmse_from_path(logs[k][0], logs[k][1], wp)
    return out


def f0_contour_rmse(f0_ref, f0_sys, method: str = "fastdtw", radius: int = 25, engine=None, dtw_series=None) -> float:
    return f0_contour_rmse_batch([(f0_ref, f0_sys)], method, radius, engine, dtw_series)[0]


def to_pcm16(y) -> np.ndarray:
    """int16 samples as they are; floating-point audio (``librosa.load``'s [-1, 1)) scaled by 32768, rounded and clipped."""
    y = np.asarray(y)
    if y.ndim > 1:
        y = y.mean(axis=0) if y.shape[0] < y.shape[-1] else y.mean(axis=-1)        # librosa.to_mono
    if np.issubdtype(y.dtype, np.floating):
        return np.clip(np.rint(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return np.ascontiguousarray(y, dtype=np.int16)


def _check_f0(f0: str, crepe_weights):
    if f0 not in ("pyin", "crepe"):
        raise ValueError('f0: "pyin" or "crepe"')
    if f0 == "crepe" and crepe_weights is None:
        raise ValueError('f0="crepe" needs crepe_weights=: the path of a torchcrepe checkpoint (full.pth / tiny.pth), its state_dict, or '
                         '(c_out, flat vector) from crepe_weights.fold -- no trained CREPE weights ship with this project')


def _crepe_ensure(engine, model, weights):
    """Load ``weights`` (a checkpoint path, a ``state_dict``, or ``(c_out, flat)``) into ``engine`` unless the same object already is."""
    from .. import crepe_weights as CW
    _check_f0("crepe", weights)
    key = (weights if isinstance(weights, (str, Path)) else id(weights), model)
    if getattr(engine, "_crepe_key", None) == key:
        return
    if isinstance(weights, (str, Path)):
        c_out, flat = CW.load(weights)
    elif isinstance(weights, dict):
        c_out, flat = CW.fold(weights)
    else:
        c_out, flat = weights
    if model is not None and tuple(CW.dims(model)) != tuple(c_out):
        raise ValueError(f"model={model!r} has widths {CW.dims(model)}, the weights have {tuple(c_out)}")
    engine.crepe_load(c_out, flat)
    engine._crepe_key = key
    engine._crepe_keep = weights                                    # (keeps id(weights) from being reused while it is the key)


def extract_f0_torchcrepe_batch(engine, clips, sr: int, hop_length: int = 512, fmin: float = None, fmax: float = None, model: str = "full",
                                threshold: float = 0.1, batch_size: int = 4096, weights=None, decoder: str = "viterbi",
                                return_periodicity: bool = False):
    """Batched ``extract_f0_torchcrepe``: ``torchcrepe.predict(audio, sr, hop_length, fmin, fmax, model, batch_size=batch_size,
    return_periodicity=True)`` of every clip (all at rate ``sr``), then ``f0[periodicity < threshold] = NaN`` -> F0 contours in Hz.  Clips at
    another rate than 16 kHz go through ``_resample_batch`` and the hop becomes ``int(hop_length * 16000 / sr)``, as in torchcrepe."""
    from .. import crepe_weights as CW
    engine = _engine(engine)
    _crepe_ensure(engine, model, weights)
    fmin = C2_HZ if fmin is None else fmin
    fmax = C6_HZ if fmax is None else fmax
    pcm = _resample_batch(engine, clips, [int(sr)] * len(clips), CW.SAMPLE_RATE)
    engine.upload(pcm, CW.SAMPLE_RATE)
    _, f0s, pers = engine.crepe(CW.hop_at_16k(hop_length, sr), fmin, fmax, decoder, batch_size)
    out = [np.where(p < threshold, np.nan, f) for f, p in zip(f0s, pers)]
    return (out, pers) if return_periodicity else out


def extract_f0_torchcrepe(y, sr: int, hop_length: int = 512, fmin: float = None, fmax: float = None, model: str = "full", threshold: float = 0.1,
                          batch_size: int = 4096, engine=None, weights=None) -> np.ndarray:
    """The notebook's ``extract_f0_torchcrepe(y, sr, ...)`` (its ``device`` argument is the engine's): F0 in Hz, NaN where the periodicity is
    below ``threshold``.  ``weights``: see ``_crepe_ensure``."""
    return extract_f0_torchcrepe_batch(engine, [y], sr, hop_length, fmin, fmax, model, threshold, batch_size, weights)[0]


def extract_f0_batch(engine, clips, sr: int, hop_length: int = 512, fmin: float = None, fmax: float = None, f0: str = "pyin",
                     crepe_weights=None, crepe_model: str = None, crepe_threshold: float = 0.1) -> List[np.ndarray]:
    """F0 contours (Hz, NaN where unvoiced) of ``clips`` -- ``f0="pyin"``: ONE upload, one probabilistic-YIN run (``librosa.pyin`` with its
    default frame length 2048, the notebook's stated F0 step); ``f0="crepe"``: ``extract_f0_torchcrepe_batch`` (the notebook's code; see the
    module text)."""
    _check_f0(f0, crepe_weights)
    if f0 == "crepe":
        return extract_f0_torchcrepe_batch(engine, clips, sr, hop_length, fmin, fmax, crepe_model, crepe_threshold, weights=crepe_weights)
    from ..visualisation.acoustic_analysis import pyin_batch
    fmin = C2_HZ if fmin is None else fmin
    fmax = C6_HZ if fmax is None else fmax
    engine.upload([to_pcm16(c) for c in clips], int(sr))
    return [f0 for f0, _, _ in pyin_batch(engine, fmin, fmax, hop_length)]


def compute_f0_rmse_batch(engine, episodes, sr: int, hop_length: int = 512, fmin: float = None, fmax: float = None, method: str = "fastdtw",
                          radius: int = 25, f0: str = "pyin", crepe_weights=None, crepe_threshold: float = 0.1) -> List[float]:
    """``compute_f0_rmse`` of every ``(y_ref, y_sys)`` of ``episodes`` (all at rate ``sr``): all recordings are clips of one upload, all
    DTWs one batch.  ``f0``: ``"pyin"`` or ``"crepe"`` (with ``crepe_weights``; frames whose periodicity is below
    ``crepe_threshold`` are unvoiced), see ``extract_f0_batch``."""
    _check_f0(f0, crepe_weights)
    engine = _engine(engine)
    if not len(episodes):
        return []
    f0 = extract_f0_batch(engine, [y for ep in episodes for y in ep], sr, hop_length, fmin, fmax, f0, crepe_weights,
                          crepe_threshold=crepe_threshold)
    return f0_contour_rmse_batch([(f0[2 * k], f0[2 * k + 1]) for k in range(len(episodes))], method, radius, engine)


def compute_f0_rmse(engine, y_ref, y_sys, sr: int, hop_length: int = 512, fmin: float = None, fmax: float = None, method: str = "fastdtw",
                    radius: int = 25, f0: str = "pyin", crepe_weights=None, crepe_threshold: float = 0.1) -> float:
    """RMSE of log-F0 between a recording and a synthesis at the same rate ``sr``: F0 of both by the engine's pYIN (``f0="pyin"``, the
    default) or its CREPE (``f0="crepe"`` with ``crepe_weights``: the notebook's code path, module text) -- two clips of one upload;
    ``fmin`` / ``fmax`` default to C2 / C6 as the notebook sets them --, voiced frames only, natural log, DTW (``method="fastdtw"``
    with ``radius``, or ``"exact"``), then ``sqrt(mean((log_r[wp[:, 0]] - log_s[wp[:, 1]]) ** 2))`` on the fetched path.  NaN when
    either side has no voiced frame."""
    return compute_f0_rmse_batch(engine, [(y_ref, y_sys)], sr, hop_length, fmin, fmax, method, radius, f0, crepe_weights, crepe_threshold)[0]


# --------------------------------------------------------------------------------------------------------- WER
def wer_words(text: str) -> List[str]:
    """jiwer's default transform of one sentence: ``RemoveMultipleSpaces`` (``re.sub(r"\\s\\s+", " ", s)``), ``Strip``, split on
    ``" "`` dropping empty strings."""
    return [w for w in re.sub(r"\s\s+", " ", text).strip().split(" ") if w]


def compute_wer_batch(pairs, engine=None, edit_distance=None) -> List[float]:
    """``jiwer.wer(ref, sys)`` of every ``(ref_txt, sys_txt)``: ``(S + D + I) / len(reference words)``, the numerator being the
    word-level edit distance (``pce_levenshtein`` on integer word ids; ``edit_distance``: a callable taking [(ids_a, ids_b), ...], default
    the engine's).  An empty reference raises ValueError, as jiwer does."""
    ids, packed = {}, []
    for ref_txt, sys_txt in pairs:
        ref, hyp = wer_words(ref_txt), wer_words(sys_txt)
        if not ref:
            raise ValueError("one or more references are empty strings")
        packed.append(tuple(np.array([ids.setdefault(w, len(ids)) for w in ws], dtype=np.uint32) for ws in (ref, hyp)))
    if not packed:
        return []
    dist = (edit_distance or _engine(engine).levenshtein_ids)(packed)
    return [int(d) / len(p[0]) for d, p in zip(dist, packed)]


def compute_wer(ref_txt: str, sys_txt: str, engine=None, edit_distance=None) -> float:
    return compute_wer_batch([(ref_txt, sys_txt)], engine, edit_distance)[0]


# --------------------------------------------------------------------------------------------------------- breaks
def compute_f1_break(breaks_ref, breaks_sys, tol=0.3):
    """Match each reference break to the first unused system break within ``tol`` seconds (the notebook's greedy loop, verbatim).
    -> ``(f1, precision, recall)``."""
    tp = 0
    used_sys = set()
    for r in breaks_ref:
        for i, s in enumerate(breaks_sys):
            if i in used_sys:
                continue
            if abs(r - s) <= tol:
                tp += 1
                used_sys.add(i)
                break
    fp = len(breaks_sys) - len(used_sys)
    fn = len(breaks_ref) - tp
    prec = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    rec = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    f1 = 2 * prec * rec / (prec + rec) if (prec + rec) > 0 else 0.0
    return f1, prec, rec


class WhisperHandle:
    """What the notebook's global ``whisper_model`` is here: a checkpoint loaded into an engine, with its tokenizer."""

    def __init__(self, model, tokenizer):
        self.model, self.tokenizer = model, tokenizer

    @classmethod
    def load(cls, engine, model_size: str = "large-v3", model_dir: Optional[str] = None, language: Optional[str] = "fr"):
        """``language``: the tokenizer's own language (prompts and word splitting when a call names none); None for a handle that is only ever
        used with ``language=None`` (detection per recording)."""
        from ..Aligners import checkpoint as CK
        model = CK.load_model(model_size, model_dir).load_into(engine)
        return cls(model, CK.load_tokenizer(model_dir, language, model.text_dims["n_vocab"]))


def _resample_batch(engine, clips, rates, target: int) -> List[np.ndarray]:
    """Every clip at ``target`` Hz; clips of one source rate are one upload through the engine's polyphase resampler."""
    out = [None] * len(clips)
    for r in sorted(set(rates)):
        idx = [i for i, x in enumerate(rates) if x == r]
        if r == target:
            for i in idx:
                out[i] = to_pcm16(clips[i])
            continue
        engine.upload([to_pcm16(clips[i]) for i in idx], int(r))
        engine.resample(int(target))
        for i, y in zip(idx, engine.download()):
            out[i] = y
    return out


def _load(audio):
    if isinstance(audio, (str, Path)):
        rate, pcm = H.decode_wav(audio)
        return pcm, rate
    pcm, rate = audio
    return to_pcm16(pcm), int(rate)


def extract_transcripts_and_breaks(engine, model: WhisperHandle, audios, language: Optional[str] = "fr"):
    """Batched ``extract_transcript_and_breaks``: ``audios`` = paths of 16-bit WAV files or ``(samples, rate)`` -> one
    ``(text, breaks, segments)`` per recording, all recordings one transcription batch.  ``language=None``: detected per recording
    (recordings of different languages share the batch)."""
    from ..Aligners import transcribe as TR
    engine = _engine(engine)
    loaded = [_load(a) for a in audios]
    clips = _resample_batch(engine, [p for p, _ in loaded], [r for _, r in loaded], TR.SAMPLE_RATE)
    # the notebook calls plain ``whisper_timestamped``'s ``model.transcribe(path)``: no VAD, no disfluency marks
    opts = TR.TranscribeOptions(language=language, vad=None, detect_disfluencies=False)
    out = []
    for result in TR.transcribe_batch(engine, model.model, model.tokenizer, clips, opts):
        text = result["text"].strip()
        breaks = [seg["end"] for seg in result["segments"][:-1]]
        segments = [{"start": seg["start"], "end": seg["end"], "text": seg["text"].strip()} for seg in result["segments"]]
        out.append((text, breaks, segments))
    return out


def extract_transcript_and_breaks(engine, model: WhisperHandle, audio, language: Optional[str] = "fr"):
    """Transcript, phrase-break times (the end of every segment but the last) and segments of one recording, through
    ``Aligners/transcribe.py`` with ``vad=None``.  The language is an argument; None detects it, as the notebook's ``model.transcribe(path)`` does."""
    return extract_transcripts_and_breaks(engine, model, [audio], language)[0]


# --------------------------------------------------------------------------------------------------------- driver
SIDE_FILES = ("reference.wav", "reference_transcript.txt", "reference_breaks.txt", "reference_segments.json",
              "synthetic.wav", "synthetic_transcript.txt", "synthetic_breaks.txt", "synthetic_segments.json")


def _write_wav(path: Path, pcm: np.ndarray, rate: int):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(rate)); w.writeframes(np.asarray(pcm, dtype="<i2").tobytes())


def _write_side(save_path: Path, prefix: str, txt: str, breaks, segments):
    (save_path / f"{prefix}_transcript.txt").write_text(txt, encoding="utf-8")
    (save_path / f"{prefix}_breaks.txt").write_text("\n".join(map(str, breaks)), encoding="utf-8")
    with open(save_path / f"{prefix}_segments.json", "w", encoding="utf-8") as f:
        json.dump(segments, f)


def process_episodes(ep_ids: Sequence[str], voice_base, results_base, save_dir, engine=None, model: WhisperHandle = None, language: Optional[str] = "fr",
                     method: str = "fastdtw", radius: int = 25, f0: str = "pyin", crepe_weights=None):
    """``process_episode`` for a list of episodes, stage by stage over all of them -> [(ep_id, rmse_f0, f1_break, wer, error | None)].
    Folder contract of the notebook: ``{voice_base}/{ep}/brute/segment_demucs.wav`` is the reference, ``{results_base}/{ep}/OUT.wav`` the
    synthesis (resampled to the reference's rate by the engine's resampler), the side files go to ``{save_dir}/{ep}/``."""
    _check_f0(f0, crepe_weights)
    engine = _engine(engine)
    if model is None:
        raise ValueError("model: a WhisperHandle (WhisperHandle.load(engine, 'large-v3', model_dir))")
    vb, rb = Path(voice_base), Path(results_base)
    out = {ep: None for ep in ep_ids}
    ref, syn = {}, {}
    for ep in ep_ids:
        save_path = Path(save_dir) / ep
        save_path.mkdir(parents=True, exist_ok=True)
        try:
            demucs_path = vb / ep / "brute" / "segment_demucs.wav"
            if not demucs_path.exists():
                raise FileNotFoundError(f"No demucs file at {demucs_path}")
            sr_ref, y_ref = H.decode_wav(demucs_path)
            _write_wav(save_path / "reference.wav", y_ref, sr_ref)
            ref[ep] = (y_ref, sr_ref)
            sys_path = rb / ep / "OUT.wav"
            if sys_path.exists():
                sr_sys, y_sys = H.decode_wav(sys_path)
                syn[ep] = (y_sys, sr_sys)
        except Exception as e:                                               # noqa: BLE001 (per-episode failures are results, as in the notebook)
            out[ep] = (ep, np.nan, np.nan, np.nan, str(e))
    have_ref = [ep for ep in ep_ids if ep in ref]
    # references are transcribed (and their side files written) even where OUT.wav is missing, as the notebook does before it looks for it
    both = [ep for ep in have_ref if ep in syn]
    for sr_ref in sorted({ref[ep][1] for ep in both}):
        eps = [ep for ep in both if ref[ep][1] == sr_ref]
        ys = _resample_batch(engine, [syn[ep][0] for ep in eps], [syn[ep][1] for ep in eps], sr_ref)
        for ep, y in zip(eps, ys):
            syn[ep] = (y, sr_ref)
            _write_wav(Path(save_dir) / ep / "synthetic.wav", y, sr_ref)
    tr = extract_transcripts_and_breaks(engine, model, [ref[ep] for ep in have_ref] + [syn[ep] for ep in both], language) if have_ref else []
    tr_ref = dict(zip(have_ref, tr[:len(have_ref)])); tr_sys = dict(zip(both, tr[len(have_ref):]))
    for ep in have_ref:
        _write_side(Path(save_dir) / ep, "reference", *tr_ref[ep])
        if ep in tr_sys:
            _write_side(Path(save_dir) / ep, "synthetic", *tr_sys[ep])
        else:
            out[ep] = (ep, np.nan, np.nan, np.nan, "Missing OUT.wav")
    rmse = {}
    for sr_ref in sorted({ref[ep][1] for ep in both}):
        eps = [ep for ep in both if ref[ep][1] == sr_ref]
        rmse.update(zip(eps, compute_f0_rmse_batch(engine, [(ref[ep][0], syn[ep][0]) for ep in eps], sr_ref, method=method, radius=radius, f0=f0,
                                                    crepe_weights=crepe_weights)))
    wers = {}
    for ep in both:                                                          # an empty reference transcript fails that episode alone
        try:
            wers[ep] = compute_wer(tr_ref[ep][0], tr_sys[ep][0], engine)
        except ValueError as e:
            out[ep] = (ep, np.nan, np.nan, np.nan, str(e))
    for ep in both:
        if ep in wers:
            f1_b, _, _ = compute_f1_break(tr_ref[ep][1], tr_sys[ep][1], tol=0.3)
            out[ep] = (ep, rmse[ep], f1_b, wers[ep], None)
    return [out[ep] for ep in ep_ids]


def process_episode(ep_id: str, voice_base, results_base, save_dir, engine=None, model: WhisperHandle = None, **kw):
    return process_episodes([ep_id], voice_base, results_base, save_dir, engine, model, **kw)[0]


def evaluate_all(voice_base, results_base, save_dir, engine=None, model: WhisperHandle = None, language: Optional[str] = "fr", method: str = "fastdtw",
                 radius: int = 25, f0: str = "pyin", crepe_weights=None):
    """Every episode folder of ``results_base`` -> ``pandas.DataFrame`` indexed by ``episode`` with ``rmse_f0``, ``f1_break``, ``wer``
    (episodes that failed -- a missing ``OUT.wav`` among them -- are reported and left out, as in the notebook).  All episodes form one
    batch per stage.  Under an initialised ``torch.distributed`` group every rank takes a contiguous block of the episodes
    (``shard.shard_range``) and the rows are exchanged with ``shard.allgather_records``: every rank returns the whole table."""
    _check_f0(f0, crepe_weights)
    import pandas as pd
    from .. import shard
    ep_ids = sorted(p.name for p in Path(results_base).iterdir() if p.is_dir())
    rank, world = shard.rank_world()
    lo, hi = shard.shard_range(len(ep_ids), rank, world)
    rows, failed = [], False
    try:
        for k, (ep, rmse, f1_b, wer_score, err) in zip(range(lo, hi), process_episodes(ep_ids[lo:hi], voice_base, results_base, save_dir, engine, model,
                                                                                      language, method, radius, f0, crepe_weights)):
            if err:
                print(f"❌ {ep}: {err}")
            else:
                print(f"✅ {ep}: RMSE={rmse:.3f}, F1_break={f1_b:.3f}, WER={wer_score:.3f}")
            rows.append((k, 0.0 if err else 1.0, rmse, f1_b, wer_score))
    except Exception:                                                        # noqa: BLE001
        if not shard.exchanging():
            raise
        failed = True                                                        # the other ranks must not wait inside the exchange
    counts = [b - a for a, b in (shard.shard_range(len(ep_ids), r, world) for r in range(world))]
    table = shard.allgather_records(np.array(rows, dtype=np.float64).reshape(-1, 5), counts if shard.exchanging() else None, failed=failed)
    records = [{"episode": ep_ids[int(r[0])], "rmse_f0": r[2], "f1_break": r[3], "wer": r[4]} for r in table if r[1] == 1.0]
    df = pd.DataFrame(records, columns=["episode", "rmse_f0", "f1_break", "wer"]).set_index("episode")
    if len(df):
        print("\nOverall metrics:")
        print(df.mean())
    return df
