"""Data side of the reference's corpus-wide comparison of natural and synthesised speech
(Code/visualisation/Compare_speech_noenhanced.py) on the engine.

The reference opens every ``segment_phN.wav`` of a database with Praat two or three times and reduces it to one number: the mean
voiced F0 (``Sound.to_pitch(time_step=0.01)``), the mean positive intensity (``Sound.to_intensity()``) or the duration.  Here the
files of the whole database are decoded once, grouped by sample rate, uploaded in bounded batches and measured in one launch per
batch (``pce_pitch_*`` / ``pce_intensity_*``); only F0 contours (pitch) or 40-byte summaries (volume) come back.  ``'rate'`` never
touches the device.  A file measured alone and the same file inside a batch give the same bits (the kernels' results do not depend
on what a clip is batched with), so the per-file functions below and :func:`extract_and_cache_feature` agree exactly.

Files are read with :func:`hostrules.decode_wav`: 16-bit PCM WAV, and of a multi-channel file the FIRST channel (Praat would average
the channels: out of scope).  The plotting functions and the command line of the reference are not built;
:func:`zscore_feature` and :func:`raw_feature` return the arrays its two curve plots draw.
"""
from __future__ import annotations

import os
import re

import numpy as np

from ..engine import SLICE_OK, IntensityParams, PitchParams, get_default_engine
from ..hostrules import PraatError, decode_wav

FEATURES = ("pitch", "volume", "rate")
MAX_BATCH_BYTES = 256 << 20          # PCM bytes resident per upload


def _measure_batch(eng, rate, clips, feature, time_step, want):
    """One upload.  ``want`` = "mean": the reference's per-file number; "contour": the analysis' own array.  -> one value or exception per clip."""
    eng.upload(clips, rate)
    sl = eng.whole_clip_slices()
    if feature == "pitch":
        res = eng.pitch(sl, PitchParams.praat(75.0, 600.0, time_step))
        arr, off, summ = res["f0"], res["frame_offsets"], res["summary"]
    else:
        res = eng.intensity(sl, IntensityParams.praat(), want_contour=(want == "contour"))
        arr, off, summ = res["values"], res["frame_offsets"], res["summary"]
    out = []
    for i in range(len(clips)):
        if summ["status"][i] != SLICE_OK:
            out.append(PraatError("Sound shorter than the analysis window." if len(clips[i]) else "Sound contains no samples."))
        elif want == "contour":
            out.append(arr[off[i]:off[i + 1]].copy())
        elif feature == "pitch":
            f0 = arr[off[i]:off[i + 1]]
            voiced = f0[f0 > 0]
            out.append(float(np.nanmean(voiced)) if len(voiced) else float("nan"))
        else:
            out.append(float(summ["mean_positive"][i]) if summ["n_positive"][i] else float("nan"))
    return out


def measure_files(paths, feature, engine=None, time_step=0.01, want="mean", max_batch_bytes=MAX_BATCH_BYTES):
    """``feature`` ('pitch' | 'volume') of every file in ``paths`` -> {path: value, or the exception that file raised}.  Files are decoded in
    the given order, collected per sample rate and measured whenever a rate's pending clips reach ``max_batch_bytes``."""
    eng = engine or get_default_engine()
    results, pending = {}, {}

    def flush(rate):
        names, clips = pending.pop(rate)
        for name, val in zip(names, _measure_batch(eng, rate, clips, feature, time_step, want)):
            results[name] = val

    for path in dict.fromkeys(paths):
        try:
            rate, pcm = decode_wav(path)
        except Exception as e:                                  # the reference catches every exception per pair
            results[path] = e
            continue
        names, clips = pending.setdefault(rate, ([], []))
        names.append(path); clips.append(pcm)
        if 2 * sum(len(c) for c in clips) >= max_batch_bytes:
            flush(rate)
    for rate in list(pending):
        flush(rate)
    return results


def _one(path, feature, engine, **kw):
    val = measure_files([path], feature, engine, **kw)[path]
    if isinstance(val, Exception):
        raise val
    return val


def extract_pitch_mean(audio_path, time_step=0.01, engine=None):
    """Mean of the voiced frames of ``Sound.to_pitch(time_step)`` (floor 75 Hz, ceiling 600 Hz), NaN when none is voiced."""
    return _one(audio_path, "pitch", engine, time_step=time_step)


def extract_mean_volume(audio_path, engine=None):
    """Mean of the positive values of ``Sound.to_intensity()``, NaN when there are none."""
    return _one(audio_path, "volume", engine)


def extract_duration(audio_path):
    """``Sound.get_total_duration()``: samples over sample rate.  Host only."""
    rate, pcm = decode_wav(audio_path)
    return len(pcm) / rate


def compare_pitch(naturelle_dir, synthese_dir, engine=None):
    """Mean pitch of every WAV name the two directories share -> (natural, synthesis, names), NaN pairs dropped, failing pairs reported."""
    is_wav = lambda f: f.lower().endswith(".wav")
    common = sorted(set(filter(is_wav, os.listdir(naturelle_dir))) & set(filter(is_wav, os.listdir(synthese_dir))))
    pairs = [(os.path.join(naturelle_dir, f), os.path.join(synthese_dir, f)) for f in common]
    vals = measure_files([p for pair in pairs for p in pair], "pitch", engine)
    nat_out, syn_out, labels = [], [], []
    for fname, (nat_path, syn_path) in zip(common, pairs):
        nat, syn = vals[nat_path], vals[syn_path]
        err = nat if isinstance(nat, Exception) else syn if isinstance(syn, Exception) else None
        if err is not None:
            print(f"Erreur avec {fname}: {err}")
        elif not (np.isnan(nat) or np.isnan(syn)):
            nat_out.append(nat); syn_out.append(syn); labels.append(fname)
    return nat_out, syn_out, labels


def list_segment_pairs(root_dir):
    """The reference's walk over a database: every directory entry ``<speaker>[_EPnn]`` that has an ``audio`` folder and a sibling
    ``<entry>_microsoft/audio``, in ``os.listdir`` order; inside, the ``segment_phN.wav`` files present on both sides, sorted by name.
    -> [(natural path, synthesis path, speaker, sample id)]."""
    pairs = []
    for entry in os.listdir(root_dir):
        if not os.path.isdir(os.path.join(root_dir, entry)):
            continue
        m = re.match(r"(.+?)(_EP\d+)?$", entry)
        if not m:
            continue
        speaker, episode = m.group(1), m.group(2) or ""
        nat_dir = os.path.join(root_dir, entry, "audio")
        syn_dir = os.path.join(root_dir, entry + "_microsoft", "audio")
        if not (os.path.isdir(nat_dir) and os.path.isdir(syn_dir)):
            continue
        is_segment = lambda f: f.startswith("segment_ph") and f.endswith(".wav")
        syn_names = set(filter(is_segment, os.listdir(syn_dir)))
        for seg in sorted(filter(is_segment, os.listdir(nat_dir))):
            num = re.match(r"segment_ph(\d+)\.wav", seg)
            if not num:
                continue
            partner = f"segment_ph{num.group(1)}.wav"
            if partner in syn_names:
                pairs.append((os.path.join(nat_dir, seg), os.path.join(syn_dir, partner), speaker, f"{speaker}{episode}_ph{num.group(1)}"))
    return pairs


def extract_and_cache_feature(root_dir, feature, engine=None, max_batch_bytes=MAX_BATCH_BYTES):
    """``feature`` in 'pitch' | 'volume' | 'rate' for every natural / synthesis pair of the database -> (natural, synthesis, speakers,
    sample ids) in the reference's order.  A pair with a NaN is dropped; a pair one of whose files cannot be read or is shorter than the
    analysis window (Praat raises there) is reported with the reference's ``Erreur avec ...`` line and skipped."""
    naturelle, synthese, speakers, samples = [], [], [], []
    if feature not in FEATURES:
        return naturelle, synthese, speakers, samples
    pairs = list_segment_pairs(root_dir)
    if feature == "rate":
        vals = {}
        for path in dict.fromkeys(p for pair in pairs for p in pair[:2]):
            try:
                dur = extract_duration(path)
                vals[path] = 1.0 / dur if dur > 0 else float("nan")
            except Exception as e:
                vals[path] = e
    else:
        vals = measure_files([p for pair in pairs for p in pair[:2]], feature, engine, max_batch_bytes=max_batch_bytes)
    for nat_path, syn_path, speaker, sample_id in pairs:
        nat, syn = vals[nat_path], vals[syn_path]
        err = nat if isinstance(nat, Exception) else syn if isinstance(syn, Exception) else None
        if err is not None:
            print(f"Erreur avec {nat_path} ou {syn_path}: {err}")
            continue
        if np.isnan(nat) or np.isnan(syn):
            continue
        naturelle.append(nat); synthese.append(syn); speakers.append(speaker); samples.append(sample_id)
    return naturelle, synthese, speakers, samples


def save_feature_only(filepath, naturelle, synthese, speakers, samples):
    np.savez(filepath, naturelle=naturelle, synthese=synthese, speakers=speakers, samples=samples)


def load_feature_only(filepath):
    with np.load(filepath, allow_pickle=True) as data:
        return tuple(data[k].tolist() for k in ("naturelle", "synthese", "speakers", "samples"))


def print_quartiles(naturelle_pitches, synthese_pitches):
    for title, values in (("Voix naturelle :", naturelle_pitches), ("Voix synthèse :", synthese_pitches)):
        q1, med, q3 = np.percentile(np.array(values), [25, 50, 75])
        print(title)
        print(f"  Q1 (25%)   : {q1:.2f} Hz")
        print(f"  Médiane    : {med:.2f} Hz")
        print(f"  Q3 (75%)   : {q3:.2f} Hz")


def raw_feature(nat_path, syn_path, feature, engine=None):
    """The two arrays ``plot_raw_feature`` draws: the F0 contour of ``to_pitch()`` or the contour of ``to_intensity()`` with the
    values ``<= 0`` removed, or, for 'rate', the constant ``1 / duration`` once per pitch frame.  None for an unknown feature."""
    if feature not in FEATURES:
        print("Feature inconnue pour la courbe brute. Utilisez pitch, volume ou rate.")
        return None
    vals = measure_files([nat_path, syn_path], "volume" if feature == "volume" else "pitch", engine, time_step=0.0, want="contour")
    out = []
    for path in (nat_path, syn_path):
        arr = vals[path]
        if isinstance(arr, Exception):
            raise arr
        out.append(np.ones_like(arr) * (1.0 / extract_duration(path)) if feature == "rate" else arr[arr > 0])
    return tuple(out)


def zscore_feature(nat_path, syn_path, feature, engine=None):
    """The two arrays ``plot_zscore_feature`` draws: :func:`raw_feature`, each standardised by its own mean and standard deviation when it
    has more than one value."""
    if feature not in FEATURES:
        print("Feature inconnue pour la variabilité. Utilisez pitch, volume ou rate.")
        return None
    with np.errstate(divide="ignore", invalid="ignore"):      # 'rate' is constant: 0 / 0, as in the reference
        return tuple((a - np.mean(a)) / np.std(a) if len(a) > 1 else a for a in raw_feature(nat_path, syn_path, feature, engine))
