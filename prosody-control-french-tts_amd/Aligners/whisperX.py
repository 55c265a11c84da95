"""Mirror of ``Code/Aligners/whisperX.py`` without its import-time ``sys.argv`` block: transcribe a directory of recordings, align every
transcript segment to the audio with a CTC acoustic model the way ``whisperx.align`` does, and write each file's ``word_segments`` as a
``Mots`` tier.

The reference calls ``whisperx.align`` once per file, and whisperx runs its trellis and back-track one segment at a time as Python loops over
torch rows; here all segments of all files go through ONE ``ProsodyEngine.wx_align`` call (``pce_wx_align``: wildcard trellis, beam
back-track).  ``whisperx`` is third party and absent: its host rules are restated in ``wx_segments`` from the published source of
whisperx 3.3.x, parity unpinned; no trained alignment model is on hand, the caller brings a ``transformers`` ``...ForCTC`` model and its
``metadata = {"language", "dictionary", "type"}`` (what ``whisperx.load_align_model`` returns).  The transcript segments come from the
project's own Whisper path (``transcribe.transcribe_batch``, greedy) or from the caller; the reference's faster-whisper large-v2 int8 with
beam 5 and pyannote VAD is not built.  Sentence splitting (nltk Punkt) is not built either: each input segment is one sentence, which
leaves ``word_segments`` as they are (``wx_segments``)."""
from __future__ import annotations

import os
import sys

import numpy as np

from .. import hostrules
from ..engine import WX_OK, DeviceEmissions
from ..textgrid_io import IntervalTier, TextGrid, write_textgrid
from . import wx_segments
from .ctc_emissions import SAMPLE_RATE


def blank_id(dictionary: dict) -> int:
    """The id of ``"[pad]"`` or ``"<pad>"`` (the later entry wins, as the source's loop has it), else 0."""
    blank = 0
    for char, code in dictionary.items():
        if char in ("[pad]", "<pad>"):
            blank = code
    return blank


def _align_files(jobs, model, metadata, engine, beam_width, emissions, acoustic="torch"):
    """``jobs``: [(segments, pcm16k)] -> one ``{"segments", "word_segments"}`` per job; every alignable segment of every job in one ``wx_align``."""
    if acoustic not in ("torch", "engine"):
        raise ValueError(f"acoustic: 'torch' or 'engine', not {acoustic!r}")
    dictionary, language = metadata["dictionary"], metadata["language"]
    if metadata.get("type", "huggingface") != "huggingface":
        raise NotImplementedError("align: a transformers ...ForCTC model (metadata type 'huggingface'); torchaudio pipelines are absent")
    plan, todo = [], []                                      # per job: [(segment with clean_*, index into todo or None)]
    for jdx, (segments, pcm) in enumerate(jobs):
        max_duration = len(pcm) / SAMPLE_RATE
        rows = []
        for segment in segments:
            seg = dict(segment)
            seg["clean_char"], seg["clean_cdx"], seg["tokens"] = wx_segments.clean_segment(seg["text"], dictionary, language)
            if not seg["clean_char"]:
                print(f"whisperX: segment {seg['text']!r} holds no character to align; it keeps its own times")
                rows.append((seg, None))
            elif seg["start"] >= max_duration:
                print(f"whisperX: segment {seg['text']!r} starts at {seg['start']} s, at or beyond the audio's {max_duration} s; it keeps its own times")
                rows.append((seg, None))
            else:
                rows.append((seg, len(todo)))
                todo.append((jdx, seg))
        plan.append(rows)
    aligned = []
    if todo:
        tokens = [np.asarray(seg["tokens"], dtype=np.int32) for _, seg in todo]
        blank = blank_id(dictionary)
        if emissions is not None:
            em = emissions if isinstance(emissions, DeviceEmissions) else [np.ascontiguousarray(e, dtype=np.float32) for job in emissions for e in job]
            aligned = engine.wx_align(em, tokens, blank=blank, beam_width=beam_width)
        elif acoustic == "engine":
            from . import ctc_emissions
            em = ctc_emissions.engine_segment_emissions(engine, model, [(pcm, [seg for j, seg in todo if j == jdx]) for jdx, (_, pcm) in enumerate(jobs)])
            aligned = engine.wx_align(em, tokens, blank=blank, beam_width=beam_width)
        else:
            import torch
            from . import ctc_emissions
            parts = []
            for jdx, (_, pcm) in enumerate(jobs):
                mine = [seg for j, seg in todo if j == jdx]
                if mine:
                    parts.append(ctc_emissions.segment_emissions(model, pcm, mine, torch.device("cuda", engine.device)))
            t_max = max(int(p.shape[1]) for p, _ in parts)
            em = torch.cat([torch.nn.functional.pad(p, (0, 0, 0, t_max - int(p.shape[1]))) for p, _ in parts], dim=0).contiguous()
            aligned = engine.wx_align(em, tokens, blank=blank, beam_width=beam_width, n_frames=np.concatenate([n for _, n in parts]))
    results = []
    for rows in plan:
        out_segments = []
        for seg, k in rows:
            res = aligned[k] if k is not None else None
            if res is None:
                out_segments.append(wx_segments.unaligned(seg))
            elif res["status"] != WX_OK or len(res["path_tok"]) < 2:
                # (one frame: the source divides by T - 1 = 0; such a segment comes back unaligned here)
                print(f"whisperX: no alignment path for segment {seg['text']!r}; it keeps its own times")
                out_segments.append(wx_segments.unaligned(seg))
            else:
                chars = wx_segments.merge_repeats(res["path_tok"], res["path_lp"], "".join(seg["clean_char"]))
                out_segments.append(wx_segments.assemble(seg, chars, len(res["path_tok"]), language))
        results.append({"segments": out_segments, "word_segments": [w for s in out_segments for w in s["words"]]})
    return results


def align(segments, model, metadata, audio, engine, beam_width=2, emissions=None, acoustic="torch"):
    """``whisperx.align(segments, model, metadata, audio, device)``: ``segments`` = ``[{"start", "end", "text"}]``; ``audio``: the 16 kHz mono
    signal (int16 or float array) or the path of a WAV file; ``engine``: a ``ProsodyEngine``; ``emissions``: precomputed ``[T, V]`` float32
    log-probabilities (a list of arrays, or a ``DeviceEmissions`` of this engine), one per ALIGNABLE segment (one with a character left and a start inside the audio) in order, in place of ``model``.
    ``acoustic``: where ``model`` runs when no emissions are given: ``"torch"`` (``ctc_emissions.segment_emissions``, one forward per segment) or
    ``"engine"`` (``ctc_emissions.engine_segment_emissions``: a ``Wav2Vec2ForCTC`` on the engine's kernels, int16 audio, all segments in one call).
    A segment with no characters, one that starts at or beyond the audio's end, and one without a path come back unaligned (original times,
    no words), with a warning.  -> ``{"segments": [{"start", "end", "text", "words"}], "word_segments": [{"word", "start", "end", "score"}]}``."""
    pcm = load_audio(audio) if isinstance(audio, (str, os.PathLike)) else np.asarray(audio).reshape(-1)
    return _align_files([(segments, pcm)], model, metadata, engine, beam_width, _one_job(emissions), acoustic)[0]


def _one_job(emissions):
    return emissions if emissions is None or isinstance(emissions, DeviceEmissions) else [emissions]


def load_audio(path):
    rate, x = hostrules.decode_wav(str(path))
    if rate != SAMPLE_RATE:
        raise ValueError(f"{path}: {rate} Hz, the alignment model takes 16 kHz")
    return x


def create_textgrid(word_segments, duration, output_file):
    """Code/Aligners/whisperX.py:39-63: the tier ``Mots`` over ``[0, duration]``; an entry's times are ``start`` / ``end`` or ``start_time`` /
    ``end_time``, its mark ``word`` or ``text``; one with a missing time or with ``start >= end`` is reported and left out; the others are
    added from ``max(M, start)`` to ``end``, ``M`` being the end of the one before.  An interval the tier refuses (inverted after the
    ``max``, beyond ``duration``) raises ValueError, as ``textgrid`` does."""
    tier = IntervalTier(name="Mots", tier_min=0.0, tier_max=duration)
    M = 0
    for segment in word_segments:
        start, end = (segment.get(key, segment.get(key + "_time")) for key in ("start", "end"))
        if start is None or end is None:
            print(f"whisperX: word without a start or an end, left out: {segment}")
            continue
        if start >= end:
            print(f"whisperX: word that does not end after it starts, left out: {segment}")
            continue
        tier.add(max(M, start), end, segment.get("word", segment.get("text", "")))
        M = end
    write_textgrid(TextGrid([tier], 0.0, duration), output_file)


def _duration(result):
    if not result["segments"]:
        return 0.0
    last = result["segments"][-1]
    duration = last.get("end", last.get("end_time", None))
    return 0.0 if duration is None else duration


def _transcribe(whisper, engine, clips):
    from .transcribe import transcribe_batch
    model, tokenizer = whisper[0], whisper[1]
    options = whisper[2] if len(whisper) > 2 else None
    return [r["segments"] for r in transcribe_batch(engine, model, tokenizer, clips, options)]


def process_files(audio_dir, transcription_dir, output_dir, *, engine, align_model, metadata, whisper=None, segments=None, emissions=None, beam_width=2,
                  acoustic="torch"):
    """The reference's ``main`` for a whole directory at once: one ``.TextGrid`` per ``.wav`` of ``sorted(os.listdir(audio_dir))`` whose
    transcription file exists (the reference checks for it and never reads it: the words come from the transcription model).
    ``segments``: {file name: ``[{"start", "end", "text"}]``}, or ``whisper = (model, tokenizer[, TranscribeOptions])`` of the project's Whisper
    path (``transcribe.transcribe_batch``, greedy) to transcribe the files; ``emissions``: {file name: ``[T, V]`` arrays, one per alignable
    segment} in place of ``align_model``; ``acoustic``: as ``align`` takes it (``"engine"``: every segment of every file in one forward call).
    The grid's duration is the last aligned segment's ``end``, or 0.0.  -> {file name: word_segments}."""
    if segments is None and whisper is None:
        raise ValueError("process_files: one of whisper / segments is required")
    if align_model is None and emissions is None:
        raise ValueError("process_files: one of align_model / emissions is required")
    os.makedirs(output_dir, exist_ok=True)
    names = []
    for audio_file in sorted(os.listdir(audio_dir)):
        if not audio_file.endswith(".wav"):
            continue
        transcription_path = os.path.join(transcription_dir, audio_file.replace(".wav", ".txt"))
        if not os.path.exists(transcription_path):
            raise FileNotFoundError(f"no transcription file: {transcription_path}")
        names.append(audio_file)
    clips = [load_audio(os.path.join(audio_dir, name)) for name in names]
    per_file = [segments[name] for name in names] if segments is not None else _transcribe(whisper, engine, clips)
    results = _align_files(list(zip(per_file, clips)), align_model, metadata, engine, beam_width,
                           None if emissions is None else [emissions[name] for name in names], acoustic)
    out = {}
    for name, result in zip(names, results):
        output_path = os.path.join(output_dir, name.replace(".wav", ".TextGrid"))
        create_textgrid(result["word_segments"], _duration(result), output_path)
        print(f"Processed file : {os.path.join(audio_dir, name)} -> {output_path}")
        out[name] = result["word_segments"]
    return out


def process_file(audio_path, transcription_path, *, engine, align_model, metadata, whisper=None, segments=None, emissions=None, beam_width=2,
                 acoustic="torch"):
    """One recording -> ``(word_segments, duration)``, as the reference's ``process_file`` returns them."""
    if not os.path.exists(audio_path):
        raise FileNotFoundError(f"no audio file: {audio_path}")
    if not os.path.exists(transcription_path):
        raise FileNotFoundError(f"no transcription file: {transcription_path}")
    if segments is None and whisper is None:
        raise ValueError("process_file: one of whisper / segments is required")
    pcm = load_audio(audio_path)
    segs = segments if segments is not None else _transcribe(whisper, engine, [pcm])[0]
    result = _align_files([(segs, pcm)], align_model, metadata, engine, beam_width, _one_job(emissions), acoustic)[0]
    return result["word_segments"], _duration(result)


def main(argv=None):
    """``whisperX.py <audio_dir> <transcription_dir> <output_dir>``: the reference's command line.  The models are the caller's (no checkpoint
    ships and none can be fetched), so the command only states its usage; call ``process_files`` with an engine, a Whisper model and an
    alignment model."""
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) != 3:
        print("Usage: python whisperX.py", "<audio_dir>", "<transcription_dir>", "<output_dir>")
        return 1
    print("whisperX: no model ships with this package; call process_files(audio_dir, transcription_dir, output_dir, engine=..., "
          "align_model=..., metadata=..., whisper=(model, tokenizer)) from Python")
    return 2
