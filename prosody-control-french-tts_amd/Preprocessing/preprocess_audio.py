"""The reference's silence splitter (Code/Preprocessing/preprocess_audio.py) on the engine.

The reference loads an episode with pydub and calls ``split_on_silence(audio, min_silence_len=1000, silence_thresh=-50,
keep_silence=300)``: one ``audioop.rms`` over a one-second slice at every millisecond.  Here the recording is uploaded once,
``pce_silence_run`` makes one pass over its samples and returns the silent ranges, pydub's range rules
(``hostrules.nonsilent_from_silent`` / ``split_ranges`` / ``pydub_slice_frames``) turn them into frame ranges, and the segments are
cut from the host copy and written with stdlib ``wave``: ``libpce`` never writes audio.  :func:`segment_audio_files` does the same
for many files, grouped by (frame rate, channels) and measured in bounded batches, one run per batch.

Files are 16-bit PCM WAV with every channel kept (pydub's rms runs over all channels); anything else raises
``hostrules.CouldntDecodeError`` (the reference hands other formats to ffmpeg: out of scope).
"""
from __future__ import annotations

import logging
import os
import sys
import wave
from pathlib import Path

import numpy as np

from ..engine import get_default_engine, make_slices
from ..hostrules import decode_wav_channels, pydub_len_ms

logger = logging.getLogger(__name__)

MAX_BATCH_BYTES = 256 << 20          # PCM bytes resident per upload


class Segment:
    """What the callers of ``split_on_silence`` use of an ``AudioSegment``: the interleaved int16 samples, the frame rate, the channel
    count, ``len()`` in pydub's milliseconds and ``export`` to WAV."""

    def __init__(self, samples, frame_rate: int, channels: int = 1):
        self.samples = np.ascontiguousarray(samples, dtype=np.int16).reshape(-1)
        self.frame_rate, self.channels = int(frame_rate), int(channels)

    @property
    def n_frames(self) -> int:
        return len(self.samples) // self.channels

    def __len__(self) -> int:
        return pydub_len_ms(self.n_frames, self.frame_rate)

    def export(self, out_f, format="wav"):
        if format != "wav":
            raise ValueError(f"only 'wav' can be written, not {format!r}")
        with wave.open(os.fspath(out_f), "wb") as w:
            w.setnchannels(self.channels); w.setsampwidth(2); w.setframerate(self.frame_rate)
            w.writeframes(self.samples.astype("<i2").tobytes())
        return out_f


def _cut(samples, rate, channels, frame_ranges):
    """Frames [begin, end) of an interleaved stream; frames beyond its end are pydub's silence padding."""
    n = len(samples) // channels
    out = []
    for begin, end in frame_ranges:
        part = samples[begin * channels:min(end, n) * channels]
        if end > n:
            part = np.concatenate([part, np.zeros((end - max(begin, n)) * channels, dtype=np.int16)])
        out.append(Segment(part, rate, channels))
    return out


def _split_batch(eng, rate, channels, clips, min_silence_len, silence_thresh, keep_silence):
    eng.upload(clips, rate)
    n = len(clips)
    slices = make_slices(np.arange(n), np.zeros(n, dtype=np.int64), [len(c) for c in clips])
    _, frames = eng.split_on_silence(slices, min_silence_len=min_silence_len, silence_thresh=silence_thresh, keep_silence=keep_silence,
                                     channels=channels)
    return [_cut(c, rate, channels, f) for c, f in zip(clips, frames)]


def segment_audio_files(paths, min_silence_len=1000, silence_thresh=-50, keep_silence=300, engine=None, max_batch_bytes=MAX_BATCH_BYTES):
    """``split_on_silence`` of every file in ``paths`` -> {path: list of :class:`Segment`, or the exception that file raised}.  Files are
    decoded in the given order, collected per (frame rate, channels) and split whenever a group's pending samples reach ``max_batch_bytes``."""
    eng = engine or get_default_engine()
    results, pending = {}, {}

    def flush(key):
        names, clips = pending.pop(key)
        for name, segs in zip(names, _split_batch(eng, key[0], key[1], clips, min_silence_len, silence_thresh, keep_silence)):
            results[name] = segs

    for path in dict.fromkeys(paths):
        try:
            rate, channels, pcm = decode_wav_channels(path)
        except Exception as e:
            results[path] = e
            continue
        names, clips = pending.setdefault((rate, channels), ([], []))
        names.append(path); clips.append(pcm)
        if 2 * sum(len(c) for c in clips) >= max_batch_bytes:
            flush((rate, channels))
    for key in list(pending):
        flush(key)
    return results


def segment_audio_file(input_file, min_silence_len, silence_thresh, keep_silence, engine=None):
    """The segments of one recording, cut at its silences (at least ``min_silence_len`` ms below ``silence_thresh`` dBFS), each keeping
    ``keep_silence`` ms of the silence around it."""
    try:
        if not os.path.exists(input_file):
            raise FileNotFoundError(f"no such file: {input_file}")
        logger.info(f"splitting {input_file} on silence")
        segments = segment_audio_files([input_file], min_silence_len, silence_thresh, keep_silence, engine)[input_file]
        if isinstance(segments, Exception):
            raise segments
        logger.info(f"{len(segments)} segments")
        return segments
    except Exception as e:
        logger.error(f"splitting failed: {e}")
        raise


def save_segments(segments, output_dir, format='wav'):
    """Write segment i (from 1) as ``segment_ph<i>.wav`` into ``output_dir``, created with its parents."""
    if format != 'wav':
        raise ValueError(f"only 'wav' can be written, not {format!r}")
    try:
        Path(output_dir).mkdir(parents=True, exist_ok=True)
        logger.info(f"writing {len(segments)} segments to {output_dir}")
        for i, segment in enumerate(segments):
            segment.export(os.path.join(output_dir, f'segment_ph{i + 1}.{format}'), format=format)
    except Exception as e:
        logger.error(f"writing the segments failed: {e}")
        raise


def analyze_segment_lengths(segments):
    """Count, mean, shortest, longest and total duration of the segments, in seconds."""
    try:
        lengths = [len(segment) for segment in segments]
        return {
            'nombre_segments': len(segments),
            'duree_moyenne': np.mean(lengths) / 1000,
            'duree_min': min(lengths) / 1000,
            'duree_max': max(lengths) / 1000,
            'duree_totale': sum(lengths) / 1000,
        }
    except Exception as e:
        logger.error(f"segment statistics failed: {e}")
        raise


def main(input_file, output_dir, min_silence_len=1000, silence_thresh=-50, keep_silence=300, engine=None):
    try:
        segments = segment_audio_file(input_file, min_silence_len, silence_thresh, keep_silence, engine=engine)
        for key, value in analyze_segment_lengths(segments).items():
            logger.info(f"{key}: {value}")
        save_segments(segments, output_dir, format='wav')
    except Exception as e:
        logger.error(f"preprocessing {input_file} failed: {e}")
        raise


if __name__ == "__main__":
    if len(sys.argv) != 3:
        print("usage: preprocess_audio.py INPUT.wav OUTPUT_DIR")
        sys.exit(1)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s - %(levelname)s - %(message)s')
    main(sys.argv[1], sys.argv[2])
