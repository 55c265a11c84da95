"""CREPE checkpoints for ``pce_crepe_load`` (include/pce.h, "CREPE pitch tracking"), and the host constants of the model.

torchcrepe's ``full.pth`` / ``tiny.pth`` are ``state_dict``s of its ``Crepe`` module; no trained checkpoint ships with this project (a user
brings their own file).  Keys: ``conv{i}.weight`` [out, in, taps, 1], ``conv{i}.bias``, ``conv{i}_BN.{weight, bias, running_mean,
running_var}`` for i = 1..6, ``classifier.{weight, bias}``.  ``fold`` turns one into the flat float32 vector the library reads: per block
the conv weight as [out][taps][in], the bias, and BatchNorm in inference form as (scale, shift), folded in float64.  BatchNorm is NOT
folded into the convolution: the block is conv, ReLU, BatchNorm, max-pool in that order, and the scale may be negative.
"""
from __future__ import annotations

import math

import numpy as np

SAMPLE_RATE = 16000
WINDOW_SIZE = 1024
PITCH_BINS = 360
CENTS_PER_BIN = 20
CENTS_OFFSET = 1997.3794084376191            # bin 0, in cents above 10 Hz
BN_EPS = 0.0010000000474974513
TAPS = (512, 64, 64, 64, 64, 64)
DIMS = {"full": (1024, 128, 128, 128, 256, 512), "tiny": (128, 16, 16, 16, 32, 64)}


def dims(capacity_or_dims):
    """``"full"`` / ``"tiny"`` or six output widths -> the six output widths."""
    if isinstance(capacity_or_dims, str):
        if capacity_or_dims not in DIMS:
            raise ValueError(f'CREPE capacity {capacity_or_dims!r}: "full" or "tiny" (or six output widths)')
        return tuple(DIMS[capacity_or_dims])
    c_out = tuple(int(x) for x in capacity_or_dims)
    if len(c_out) != 6:
        raise ValueError("six output widths")
    return c_out


def in_channels(c_out):
    return (1,) + tuple(c_out[:-1])


def n_embedding(c_out) -> int:
    return 4 * c_out[5]                       # 1024 samples -> 256 (stride 4) -> six pools of 2 -> 4 time steps


def state_dict_shapes(capacity_or_dims):
    """[(key, shape), ...] of the module's ``state_dict`` (``num_batches_tracked`` left out: ``fold`` ignores it)."""
    c_out = dims(capacity_or_dims); c_in = in_channels(c_out)
    out = []
    for i in range(6):
        out.append((f"conv{i + 1}.weight", (c_out[i], c_in[i], TAPS[i], 1)))
        out.append((f"conv{i + 1}.bias", (c_out[i],)))
        for k in ("weight", "bias", "running_mean", "running_var"):
            out.append((f"conv{i + 1}_BN.{k}", (c_out[i],)))
    out.append(("classifier.weight", (PITCH_BINS, n_embedding(c_out))))
    out.append(("classifier.bias", (PITCH_BINS,)))
    return out


def tensor_order(capacity_or_dims):
    """[(name, shape), ...] of the flat vector ``pce_crepe_load`` takes."""
    c_out = dims(capacity_or_dims); c_in = in_channels(c_out)
    out = []
    for i in range(6):
        out += [(f"conv{i + 1}.weight[out][taps][in]", (c_out[i], TAPS[i], c_in[i])), (f"conv{i + 1}.bias", (c_out[i],)),
                (f"conv{i + 1}_BN.scale", (c_out[i],)), (f"conv{i + 1}_BN.shift", (c_out[i],))]
    out += [("classifier.weight", (PITCH_BINS, n_embedding(c_out))), ("classifier.bias", (PITCH_BINS,))]
    return out


def n_floats(capacity_or_dims) -> int:
    return sum(int(np.prod(s)) for _, s in tensor_order(capacity_or_dims))


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def fold_parts(state_dict):
    """-> (c_out, [ (w [out][taps][in], bias, scale, shift) x 6 ], classifier weight, classifier bias), all float64."""
    c_out = tuple(int(_np(state_dict[f"conv{i + 1}.bias"]).shape[0]) for i in range(6))
    want = dict(state_dict_shapes(c_out))
    blocks = []
    for i in range(6):
        for k in (f"conv{i + 1}.weight", f"conv{i + 1}.bias", f"conv{i + 1}_BN.weight", f"conv{i + 1}_BN.bias", f"conv{i + 1}_BN.running_mean",
                  f"conv{i + 1}_BN.running_var"):
            if k not in state_dict:
                raise KeyError(f"CREPE state dict lacks {k}")
            if tuple(_np(state_dict[k]).shape) != want[k]:
                raise ValueError(f"{k}: shape {tuple(_np(state_dict[k]).shape)}, expected {want[k]}")
        w = _np(state_dict[f"conv{i + 1}.weight"]).astype(np.float64)[:, :, :, 0]               # [out, in, taps]
        gamma = _np(state_dict[f"conv{i + 1}_BN.weight"]).astype(np.float64)
        beta = _np(state_dict[f"conv{i + 1}_BN.bias"]).astype(np.float64)
        mean = _np(state_dict[f"conv{i + 1}_BN.running_mean"]).astype(np.float64)
        var = _np(state_dict[f"conv{i + 1}_BN.running_var"]).astype(np.float64)
        scale = gamma / np.sqrt(var + BN_EPS)
        blocks.append((np.ascontiguousarray(w.transpose(0, 2, 1)), _np(state_dict[f"conv{i + 1}.bias"]).astype(np.float64), scale, beta - mean * scale))
    cw = _np(state_dict["classifier.weight"]).astype(np.float64); cb = _np(state_dict["classifier.bias"]).astype(np.float64)
    if cw.shape != want["classifier.weight"] or cb.shape != want["classifier.bias"]:
        raise ValueError(f"classifier: shapes {cw.shape} / {cb.shape}, expected {want['classifier.weight']} / {want['classifier.bias']}")
    return c_out, blocks, cw, cb


def fold(state_dict):
    """``state_dict`` -> (c_out, flat float32 vector in ``tensor_order``)."""
    c_out, blocks, cw, cb = fold_parts(state_dict)
    parts = [a.reshape(-1) for blk in blocks for a in blk] + [cw.reshape(-1), cb]
    flat = np.concatenate(parts).astype(np.float32)
    assert flat.size == n_floats(c_out)
    return c_out, flat


def unfold(c_out, flat):
    """The flat vector cut back into ([(w [out][taps][in], bias, scale, shift) x 6], classifier weight, classifier bias), float32 views."""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    if flat.size != n_floats(c_out):
        raise ValueError(f"CREPE weight vector has {flat.size} floats, expected {n_floats(c_out)}")
    arrs, at = [], 0
    for _, shape in tensor_order(c_out):
        n = int(np.prod(shape)); arrs.append(flat[at:at + n].reshape(shape)); at += n
    return [tuple(arrs[4 * i:4 * i + 4]) for i in range(6)], arrs[24], arrs[25]


def load(path):
    """A torchcrepe checkpoint file -> (c_out, flat float32 vector)."""
    import torch
    return fold(torch.load(path, map_location="cpu", weights_only=True))


def random_init(capacity_or_dims, seed: int = 0):
    """A seeded random ``state_dict`` (numpy arrays) for tests and tools: He-scaled conv weights so that activations keep their size through
    the six blocks, BatchNorm weights of BOTH signs (|gamma| in [0.5, 1.5]) so that the ReLU -> BatchNorm -> pool order is exercised, a classifier whose logits
    move from frame to frame (a salience that follows the input, not the bias) without saturating the fp32 sigmoid."""
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in state_dict_shapes(capacity_or_dims):
        leaf = key.split(".")[-1]
        if key.startswith("classifier"):
            sd[key] = rng.standard_normal(shape) * (3.0 / math.sqrt(shape[-1])) if leaf == "weight" else rng.standard_normal(shape) * 0.1
        elif "_BN" not in key:
            sd[key] = rng.standard_normal(shape) * math.sqrt(2.0 / (shape[1] * shape[2])) if leaf == "weight" else rng.standard_normal(shape) * 0.1
        elif leaf == "weight":
            sd[key] = rng.uniform(0.5, 1.5, shape) * np.where(rng.random(shape) < 0.3, -1.0, 1.0)
        elif leaf == "bias":
            sd[key] = rng.standard_normal(shape) * 0.2
        elif leaf == "running_mean":
            sd[key] = rng.uniform(0.1, 0.6, shape)
        else:
            sd[key] = rng.uniform(0.3, 1.2, shape)
        sd[key] = sd[key].astype(np.float32)
    return sd


# ---------------------------------------------------------------------------------------------------------------- host constants of the decoding
def frequency_to_bins(frequency: float, quantize=math.floor) -> int:
    """torchcrepe.convert.frequency_to_bins: ``quantize((1200 log2(f / 10) - 1997.3794084376191) / 20)``."""
    return int(quantize((1200.0 * math.log2(frequency / 10.0) - CENTS_OFFSET) / CENTS_PER_BIN))


def bins_to_frequency(bins):
    """``10 * 2 ** ((20 bin + 1997.3794084376191) / 1200)`` (no dither)."""
    cents = CENTS_PER_BIN * np.asarray(bins, dtype=np.float64) + CENTS_OFFSET
    return 10.0 * 2.0 ** (cents / 1200.0)


def mask_range(fmin: float, fmax: float):
    """-> (lo, hi): the salience bins outside [lo, hi) are masked (``P[:, :lo] = P[:, hi:] = -inf``), clipped to the 360 bins."""
    lo = max(0, frequency_to_bins(fmin, math.floor)); hi = min(PITCH_BINS, frequency_to_bins(fmax, math.ceil))
    if lo >= hi:
        raise ValueError(f"CREPE: no pitch bin between fmin = {fmin} and fmax = {fmax}")
    return lo, hi


def n_frames(n_samples: int, hop: int) -> int:
    return 1 + int(n_samples) // int(hop)


def hop_at_16k(hop_length: int, sr: int) -> int:
    """torchcrepe resamples to 16 kHz and scales the hop: ``int(hop_length * 16000 / sr)`` (512 at 44.1 kHz -> 185)."""
    return int(hop_length) if int(sr) == SAMPLE_RATE else int(hop_length * SAMPLE_RATE / sr)
