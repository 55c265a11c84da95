"""Mirror of ``Code/Aligners/CTCFA.py`` without its ``sys.argv`` block: CTC forced alignment of a directory of recordings against their
transcriptions, written as ``Mots`` tiers.

The reference runs the ``ctc-forced-aligner`` command once per file; here every file of the directory is aligned by ONE
``ProsodyEngine.ctc_align`` call (bounded batches of ``batch_files`` files), the emissions come from a caller-supplied ``transformers``
``...ForCTC`` model (``ctc_emissions.hf_emissions``) or are handed in, and the command's post-processing is ``ctc_segments``.  The
command leaves a ``start-end: word`` text file beside each recording; ``txt_to_textgrid`` turns it into the TextGrid, as the reference does."""
from __future__ import annotations

import os

import numpy as np

from .. import hostrules
from ..engine import DeviceEmissions
from ..textgrid_io import IntervalTier, TextGrid, write_textgrid
from . import ctc_segments
from .ctc_segments import preprocess_text  # noqa: F401  (the reference module's own function)


def txt_to_textgrid(input_file, output_file):
    """Code/Aligners/CTCFA.py:45-71: every non-empty line ``start-end: word`` becomes an interval of the tier ``Mots`` (a zero-length word
    is given 5 ms); a line of another shape, or one whose times do not convert or do not fit the tier, is reported and left out."""
    tier = IntervalTier(name="Mots", tier_min=0.0)
    with open(input_file, "r", encoding="utf-8") as f:
        for line in f:
            if not line.strip():
                continue
            parts = line.strip().split(":")
            if len(parts) != 2:
                print(f"Incorrect line format: {line}")
                continue
            bounds = parts[0].strip().split("-")
            if len(bounds) != 2:
                print(f"Incorrect time format in line: {line}")
                continue
            try:
                start, end = float(bounds[0].strip()), float(bounds[1].strip())
                if start == end:
                    end += 0.005
                tier.add(start, end, parts[1].strip())
            except ValueError:
                print(f"Time conversion error in line: {line}")
    write_textgrid(TextGrid([tier]), output_file)


def write_word_file(rows, path):
    """The text file the command leaves beside a recording: one ``start-end: word`` line per word."""
    with open(path, "w", encoding="utf-8") as f:
        for r in rows:
            f.write(f"{r['start']}-{r['end']}: {r['text']}\n")


def process_files(audio_dir, transcription_dir, output_dir, language, star_frequency, romanize, *, engine, model=None, vocab=None,
                  emissions=None, blank=0, batch_files=64, acoustic="torch"):
    """Code/Aligners/CTCFA.py:74-112 for a whole directory at once.  ``engine``: a ``ProsodyEngine``; ``model``: a ``transformers``
    ``...ForCTC`` model, run on the engine's device (``language`` only named the command's default checkpoint: the caller brings the
    model); ``vocab``: character -> index of the model's vocabulary (the star is the emissions' last column); ``emissions``:
    precomputed ``(tensor [B, T_max, V + 1], n_frames)`` in place of ``model``, one row per transcribed ``.wav`` of ``sorted(os.listdir)``.
    ``acoustic``: ``"torch"`` (the default: ``model`` runs under torch, ``ctc_emissions.hf_emissions``) | ``"engine"`` (``model``'s forward pass on
    the engine's own kernels, ``ctc_emissions.engine_emissions``: the emissions stay in device memory and the alignment reads them in place).
    ``star_frequency``: ``"segment"`` | ``"edges"``.  A clip the alignment gives no path (``status`` not 0: no frames, no characters left, fewer
    frames than characters, or a -inf score) gets an empty word file and a TextGrid whose ``Mots`` tier is empty.  -> {file name: word rows}."""
    if romanize:
        raise NotImplementedError("romanize=True needs uroman, which is absent")
    if vocab is None or (model is None and emissions is None):
        raise ValueError("process_files: vocab and one of model / emissions are required")
    if acoustic not in ("torch", "engine"):
        raise ValueError("acoustic: 'torch' or 'engine'")
    os.makedirs(output_dir, exist_ok=True)
    jobs = []
    for file_name in sorted(os.listdir(audio_dir)):
        if not file_name.endswith(".wav"):
            continue
        transcription_path = os.path.join(transcription_dir, file_name.replace(".wav", ".txt"))
        if not os.path.exists(transcription_path):
            print(f"Missing transcription file: {transcription_path}")
            continue
        with open(transcription_path, "r", encoding="utf-8") as f:
            jobs.append((file_name, f.read()))
    results = {}
    for b0 in range(0, len(jobs), batch_files):
        batch = jobs[b0:b0 + batch_files]
        pcm = []
        for file_name, _ in batch:
            rate, x = hostrules.decode_wav(os.path.join(audio_dir, file_name))
            if rate != ctc_segments.SAMPLE_RATE:
                raise ValueError(f"{file_name}: {rate} Hz, the acoustic model takes 16 kHz")
            pcm.append(x)
        if emissions is not None:
            em, n_frames = emissions[0][b0:b0 + len(batch)], np.asarray(emissions[1])[b0:b0 + len(batch)]
        elif acoustic == "engine":
            from .ctc_emissions import engine_emissions
            em, n_frames = engine_emissions(engine, model, pcm), None
        else:
            from .ctc_emissions import hf_emissions
            import torch
            em, n_frames = hf_emissions(model, pcm, torch.device("cuda", engine.device))
        on_engine = isinstance(em, DeviceEmissions)         # (it carries its own lengths)
        star_index = (em.n_cols if on_engine else int(em.shape[2])) - 1      # the column appended after the model's vocabulary
        if star_index <= max(vocab.values()):
            raise ValueError(f"vocab names index {max(vocab.values())}, the emissions hold {star_index} columns before the star")
        texts = [ctc_segments.tokenize(text, vocab, star_frequency, star_index) for _, text in batch]
        targets = [np.array([lab for word in tokens for lab in word], dtype=np.int32) for _, tokens in texts]
        aligned = engine.ctc_align(em, targets, blank=blank) if on_engine else engine.ctc_align(em.contiguous(), targets, blank=blank, n_frames=n_frames)
        for (file_name, _), (text_starred, tokens), res, x in zip(batch, texts, aligned, pcm):
            audio_path = os.path.join(audio_dir, file_name)
            rows = []
            if res["status"] == 0:
                rows = ctc_segments.align_words(res["path"], res["frame_score"], text_starred, tokens, blank, n_samples=len(x))
            ctc_output_file = audio_path.replace(".wav", ".txt")
            write_word_file(rows, ctc_output_file)
            textgrid_output_file = os.path.join(output_dir, file_name.replace(".wav", ".TextGrid"))
            txt_to_textgrid(ctc_output_file, textgrid_output_file)
            print(f"Processed file : {audio_path} -> {textgrid_output_file}")
            results[file_name] = rows
    return results
