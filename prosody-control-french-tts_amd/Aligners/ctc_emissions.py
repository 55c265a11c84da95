"""Frame-wise log-probabilities of a ``transformers`` ``...ForCTC`` model for 16 kHz clips: ``hf_emissions`` runs the caller's model under torch
(plumbing, no kernel of this project; the default), ``engine_emissions`` runs a ``Wav2Vec2ForCTC``'s forward pass on the engine's own kernels
(``pce_w2v_run``) with the same windowing and leaves the emissions in device memory.  ``segment_emissions`` is whisperX's way:
one transcript segment at a time, no windows (torch plumbing too; ``Aligners/whisperX.py``); ``engine_segment_emissions`` runs the same
segments on the engine's kernels (``pce_w2v_run_segments``), all files' segments in one call.

The windowing is that of ``ctc-forced-aligner``'s ``generate_emissions`` (third party and absent: restated from the published source,
parity unpinned): a clip is padded to a whole number of windows of ``window_s`` seconds, every window is run with ``context_s`` seconds
of audio on both sides, the context's frames (50 per second) are cut away, the windows are joined and the frames of the padding dropped.
Log-softmax in float32; one column of zeros, the ``<star>`` token, is appended after the model's vocabulary."""
from __future__ import annotations

import math

import numpy as np

SAMPLE_RATE = 16000
FRAMES_PER_SECOND = 50          # the 20 ms stride of wav2vec2's feature encoder


def time_to_frame(seconds: float) -> int:
    return int(seconds * FRAMES_PER_SECOND)


def window_plan(n_samples: int, window_s: float = 30, context_s: float = 2):
    """-> (windows, padding samples behind the clip, frames kept) of one clip."""
    window = int(window_s * SAMPLE_RATE)
    n_win = max(1, math.ceil(n_samples / window))
    extension = n_win * window - n_samples
    return n_win, extension, n_win * time_to_frame(window_s) - (time_to_frame(extension / SAMPLE_RATE) if extension > 0 else 0)


def hf_emissions(model, pcm_list, device, window_s=30, context_s=2, batch_size=4):
    """``pcm_list``: int16 (scaled by 1 / 32768) or float 1-D arrays at 16 kHz.  -> (float32 tensor ``[B, T_max, V + 1]`` on ``device``, rows
    past a clip's frames zero; ``n_frames`` int32 numpy [B]): what ``ProsodyEngine.ctc_align`` takes by pointer."""
    import torch
    import torch.nn.functional as F

    dev = torch.device(device)
    model = model.to(dev).eval()
    dtype = next(model.parameters()).dtype
    window, context = int(window_s * SAMPLE_RATE), int(context_s * SAMPLE_RATE)
    cut = time_to_frame(context_s)
    chunks, owner = [], []
    plans = []
    for ci, pcm in enumerate(pcm_list):
        x = np.asarray(pcm).reshape(-1)
        x = x.astype(np.float32) / 32768.0 if x.dtype.kind in "iu" else x.astype(np.float32)
        n_win, extension, keep = window_plan(len(x), window_s, context_s)
        plans.append((n_win, keep))
        padded = F.pad(torch.from_numpy(x), (context, context + extension))
        chunks.append(padded.unfold(0, window + 2 * context, window))
        owner += [ci] * n_win
    per_clip = [[] for _ in pcm_list]
    if chunks:
        stack = torch.cat(chunks, dim=0)
        with torch.inference_mode():
            for i in range(0, stack.shape[0], batch_size):
                logits = model(stack[i:i + batch_size].to(dev, dtype)).logits.float()
                logits = logits[:, cut:logits.shape[1] - cut + 1]                    # the context's frames leave
                if logits.shape[1] != time_to_frame(window_s):
                    raise ValueError(f"the model gives {logits.shape[1]} frames per {window_s} s window, {time_to_frame(window_s)} expected (20 ms stride)")
                for k in range(logits.shape[0]):
                    per_clip[owner[i + k]].append(logits[k])
    n_frames = np.array([keep for _, keep in plans], dtype=np.int32)
    if not len(plans):
        return torch.zeros((0, 0, 0), dtype=torch.float32, device=dev), n_frames
    V = per_clip[0][0].shape[-1]
    out = torch.zeros((len(plans), int(n_frames.max()), V + 1), dtype=torch.float32, device=dev)
    for ci, parts in enumerate(per_clip):
        em = torch.log_softmax(torch.cat(parts, dim=0)[:n_frames[ci]], dim=-1)
        out[ci, :n_frames[ci], :V] = em                                              # (the star column stays zero)
    return out.contiguous(), n_frames


def engine_emissions(engine, model, pcm_list, window_s=30, context_s=2):
    """``hf_emissions``' windows and numbers on the engine's kernels: uploads ``pcm_list`` (int16 arrays at 16 kHz) as the resident batch, loads
    ``model`` (a ``transformers`` ``Wav2Vec2ForCTC``) once per model and engine, and returns the ``DeviceEmissions`` of
    ``ProsodyEngine.w2v_emissions`` (star column appended), which ``ProsodyEngine.ctc_align`` reads in place."""
    clips = []
    for pcm in pcm_list:
        x = np.asarray(pcm).reshape(-1)
        if x.dtype.kind not in "iu":
            raise ValueError("engine_emissions: int16 samples (the resident batch is PCM)")
        clips.append(x.astype(np.int16))
    if not engine.w2v_holds(model):
        engine.w2v_load(model)
    engine.upload(clips, SAMPLE_RATE)
    return engine.w2v_emissions(window_s, context_s, star=True)


MIN_SEGMENT_SAMPLES = 400       # wav2vec2's feature encoder gives no frame for less


def segment_emissions(model, pcm16k, segments, device, batch_size=1):
    """The emissions ``whisperx.align`` computes, one transcript segment at a time (third party and absent: restated from the published source
    of whisperx 3.3.x, parity unpinned): segment ``{"start": t1, "end": t2}`` owns the samples ``int(t1 * 16000) : int(t2 * 16000)`` of the
    16 kHz mono signal ``pcm16k`` (int16, scaled by 1 / 32768, or float); fewer than 400 samples are padded with zeros to 400; the caller's
    ``transformers`` ``...ForCTC`` model runs on each segment ALONE (no padding to a common length: a segment's frames do not depend on its
    neighbours; ``batch_size`` only groups segments of equal length) and ``log_softmax`` is applied in float32.  Torch plumbing, as
    ``hf_emissions`` is.  -> (float32 tensor ``[B, T_max, V]`` on ``device``, rows past a segment's frames zero; ``n_frames`` int32 numpy
    [B]): what ``ProsodyEngine.wx_align`` takes by pointer."""
    import torch
    import torch.nn.functional as F

    dev = torch.device(device)
    model = model.to(dev).eval()
    dtype = next(model.parameters()).dtype
    x = np.asarray(pcm16k).reshape(-1)
    x = x.astype(np.float32) / 32768.0 if x.dtype.kind in "iu" else x.astype(np.float32)
    wave = torch.from_numpy(x)
    pieces = []
    for seg in segments:
        piece = wave[int(seg["start"] * SAMPLE_RATE):int(seg["end"] * SAMPLE_RATE)]
        if piece.shape[0] < MIN_SEGMENT_SAMPLES:
            piece = F.pad(piece, (0, MIN_SEGMENT_SAMPLES - piece.shape[0]))
        pieces.append(piece)
    out = [None] * len(pieces)
    by_length = {}
    for k, piece in enumerate(pieces):
        by_length.setdefault(int(piece.shape[0]), []).append(k)
    with torch.inference_mode():
        for ks in by_length.values():
            for i in range(0, len(ks), max(1, int(batch_size))):
                group = ks[i:i + max(1, int(batch_size))]
                logits = model(torch.stack([pieces[k] for k in group]).to(dev, dtype)).logits.float()
                em = torch.log_softmax(logits, dim=-1)
                for r, k in enumerate(group):
                    out[k] = em[r]
    n_frames = np.array([int(e.shape[0]) for e in out], dtype=np.int32)
    if not len(out):
        return torch.zeros((0, 0, 0), dtype=torch.float32, device=dev), n_frames
    packed = torch.zeros((len(out), int(n_frames.max()), int(out[0].shape[1])), dtype=torch.float32, device=dev)
    for k, e in enumerate(out):
        packed[k, :n_frames[k]] = e
    return packed.contiguous(), n_frames


def segment_samples(segment, n_samples: int):
    """-> ``(begin, end)``: the samples ``segment_emissions``' slice ``wave[int(start * 16000):int(end * 16000)]`` takes out of a signal of
    ``n_samples``: an end (or a start) beyond the signal is clamped to it and an end in front of the start gives an empty piece, as Python's
    slice does.  A negative time would count from the signal's END in that slice; nothing aligns such a segment on purpose: ValueError."""
    begin, end = int(segment["start"] * SAMPLE_RATE), int(segment["end"] * SAMPLE_RATE)
    if begin < 0 or end < 0:
        raise ValueError(f"segment {segment.get('text', '')!r}: negative time ({segment['start']}, {segment['end']})")
    begin = min(begin, n_samples)
    return begin, max(begin, min(end, n_samples))


def engine_segment_emissions(engine, model, jobs):
    """``segment_emissions``' segments and numbers on the engine's kernels: ``jobs`` = ``[(pcm16k int16, [{"start", "end"}, ...])]``, one entry
    per file.  Uploads the files as the resident batch, loads ``model`` (a ``transformers`` ``Wav2Vec2ForCTC``) unless the engine holds it, and
    runs every segment of every file in ONE ``ProsodyEngine.w2v_segment_emissions`` call (no star column).  -> ``DeviceEmissions``, one entry per
    segment in the order of ``jobs``, which ``ProsodyEngine.wx_align`` reads in place."""
    clips, triples = [], []
    for pcm, segments in jobs:
        x = np.asarray(pcm).reshape(-1)
        if x.dtype.kind not in "iu":
            raise ValueError("engine_segment_emissions: int16 samples (the resident batch is PCM)")
        for seg in segments:
            triples.append((len(clips), *segment_samples(seg, len(x))))
        clips.append(x.astype(np.int16))
    if not engine.w2v_holds(model):
        engine.w2v_load(model)
    engine.upload(clips, SAMPLE_RATE)
    return engine.w2v_segment_emissions(triples, MIN_SEGMENT_SAMPLES, star=False)
