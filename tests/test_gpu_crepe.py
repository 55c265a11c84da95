"""pce_crepe_* on the device against the float64 restatement (tests/crepe_restatement.py), on seeded random weights (no trained CREPE
checkpoint ships with this project; parity with torchcrepe itself is unpinned).

Shapes: one batch of three clips at 16 kHz -- 100 samples (shorter than any hop used here: one frame), 0.4 s, and a 44.1 kHz clip the engine
resampled -- at hops that give 37 frames for ``tiny`` (hop 400: 1 + 17 + 19) and 8 for ``full`` (hop 2200: 1 + 3 + 4).  ``tiny`` runs the
16-column-tile GEMM (N = 16, 32, 64) and block 1 at N = 128, ``full`` the 128-column-tile GEMM (N = 128, 256, 512; block 2 at K = 65 536) and
block 1 at N = 1024; five frames of the per-block tests give row counts that are no multiple of the 128-row tile from block 3 on (5 x 64 ...
5 x 8) and more than one tile before."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crepe_restatement as R
from prosody_control_french_tts_amd import crepe_weights as CW
from prosody_control_french_tts_amd.Pipeline import evaluate_voice as EV
from prosody_control_french_tts_amd.engine import PceError, ProsodyEngine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_FILE = os.path.join(ROOT, "profiles", "r17", "crepe_parity.txt")
SEED = 17
HOPS = {"tiny": 400, "full": 2200}
N_FRAMES = {"tiny": 37, "full": 8}
LO, HI = CW.mask_range(EV.C2_HZ, EV.C6_HZ)


@functools.lru_cache(maxsize=None)
def weights(capacity):
    return CW.fold(CW.random_init(capacity, SEED))


def _tone_noise(n, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = 9000 * np.sin(2 * np.pi * 180.0 * t * (1 + 0.2 * t)) + 4000 * np.sin(2 * np.pi * 523.0 * t) + 1500 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def clips16(engine):
    """The three clips at 16 kHz; the 44.1 kHz one through the engine's resampler (the restatement starts from ITS output: resampling is the
    engine's polyphase filter, a documented deviation from torchcrepe's resampy, and is pinned by its own tests)."""
    engine.upload([_tone_noise(20000, 44100, 3)], 44100)
    engine.resample(16000)
    c = engine.download()[0]
    assert len(c) == 7257
    return [_tone_noise(100, 16000, 1), _tone_noise(6400, 16000, 2), c]


@functools.lru_cache(maxsize=None)
def _reference(capacity, key):
    clips = _reference.clips[key]
    c_out, flat = weights(capacity)
    fr = np.concatenate([R.frames(c, HOPS[capacity]) for c in clips])
    return R.salience(fr, c_out, flat, emulate=False), R.salience(fr, c_out, flat, emulate=True)


_reference.clips = {}


def reference(capacity, clips):
    """(float64 salience, fp16-emulating salience) of the batch, computed once per capacity and shared."""
    key = tuple(len(c) for c in clips)
    _reference.clips[key] = clips
    return _reference(capacity, key)


def run(engine, capacity, clips, decoder="viterbi", frames_per_chunk=4096, hop=None):
    engine.crepe_load(*weights(capacity))
    engine.upload(clips, 16000)
    return engine.crepe(hop or HOPS[capacity], EV.C2_HZ, EV.C6_HZ, decoder, frames_per_chunk, return_salience=True)


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------------------ one block at a time
@pytest.mark.parametrize("capacity", ["tiny", "full"])
@pytest.mark.parametrize("block", [1, 2, 3, 4, 5, 6])
def test_block_against_float64(engine, capacity, block):
    """A block through pce_selftest_crepe_layer on fp16 operands against float64 on the same rounded operands.  Bound per stored element, derived:
    2^-11 |y| for the rounding of the stored fp16 value, plus K 2^-23 |scale| sum(|a| |b|) for the fp32 accumulation of K products (the larger of
    the two pooled rows', since rounding may decide which row is the maximum); the three fp32 operations of the epilogue are far inside the
    second term.  Channels 0 / 1 carry scales of opposite signs: in frame 0 the pooled maximum comes from the row with the LARGER ReLU output in
    one and from the SMALLER in the other, which only the order ReLU -> BatchNorm -> pool gives (their bias is raised so that they pass the ReLU)."""
    c_out, flat = weights(capacity)
    w, bias, scale, shift = (np.array(a) for a in CW.unfold(c_out, flat)[0][block - 1])
    scale[0], scale[1] = abs(scale[0]) + 0.25, -abs(scale[1]) - 0.25
    bias[0] = bias[1] = 4.0                                          # (above the accumulators' spread: these two channels pass the ReLU, so the pairs differ)
    rng = np.random.default_rng(100 * block + len(capacity))
    n, t_in, c_in = 5, (1024 if block == 1 else 128 >> (block - 2)), w.shape[2]
    x = rng.standard_normal((n, t_in, c_in))
    if block > 1:
        x = np.abs(x) * np.where(rng.random((1, 1, c_in)) < 0.3, -1.0, 1.0)      # what a block hands on: one sign per channel, mostly
    x16, w16 = x.astype(np.float16), w.astype(np.float16)
    got = engine.selftest_crepe_layer(block, x16, w16, bias, scale, shift).astype(np.float64)
    worst, picks = 0.0, set()
    for f in range(n):
        y, bnd = R.block_forward(x16[f].astype(np.float64), block, w16.astype(np.float64), bias.astype(np.float64), scale.astype(np.float64),
                                 shift.astype(np.float64), with_bound=True)
        allowed = 2.0 ** -11 * np.abs(y) + bnd
        err = np.abs(got[f] - y)
        worst = max(worst, float((err / allowed).max()))
        if f == 0:
            for ch in (0, 1):
                r = np.maximum(R.im2row(x16[f].astype(np.float64), block) @ w16[ch].astype(np.float64).reshape(-1) + bias[ch], 0.0)
                differ = r[0::2] != r[1::2]
                took_larger = (np.maximum(r[0::2], r[1::2]) * scale[ch] + shift[ch] == y[:, ch])
                picks.add((ch, bool(took_larger[differ].all()), bool((~took_larger[differ]).all()), bool(differ.any())))
    print(f"crepe block {block} {capacity}: worst error / bound = {worst:.3f}")
    assert got.shape == (n, 128 if block == 1 else t_in // 2, w.shape[0])
    assert picks == {(0, True, False, True), (1, False, True, True)}
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("capacity", ["tiny", "full"])
def test_salience_against_float64(engine, clips16, capacity):
    """The bound is measured, not chosen: d_emul = the relative L2 distance between the restatement that rounds to fp16 where the device stores
    fp16 and the plain float64 one (both on the CPU); the device may be 4 x as far from float64 (the margin: fp32 accumulation in another order,
    fp32 sigmoid).  Both distances go to profiles/r17/crepe_parity.txt on the first GPU run.  Measured on an MI355X (seed 17): see that file."""
    ref, emul = reference(capacity, clips16)
    _, _, _, sal = run(engine, capacity, clips16)
    got = np.concatenate(sal)
    assert got.shape == ref.shape == (N_FRAMES[capacity], 360) and [len(s) for s in sal][0] == 1
    d_emul, d_dev, d_dev_emul = rel_l2(emul, ref), rel_l2(got, ref), rel_l2(got, emul)
    line = f"{capacity}: frames {len(ref)}  d_emul {d_emul:.6e}  d_device {d_dev:.6e}  d_device_to_emul {d_dev_emul:.6e}  bound 4 d_emul {4 * d_emul:.6e}"
    print("crepe salience", line)
    try:
        have = open(PARITY_FILE, encoding="utf-8").read() if os.path.exists(PARITY_FILE) else ""
        if f"{capacity}:" not in have:
            os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
            with open(PARITY_FILE, "a", encoding="utf-8") as fh:
                if not have:
                    fh.write("# tests/test_gpu_crepe.py::test_salience_against_float64, random weights (crepe_weights.random_init, seed 17):\n"
                             "# relative L2 distances of the salience [frames, 360] to the float64 restatement\n")
                fh.write(line + "\n")
    except OSError:
        pass                                                        # (a read-only checkout: the figures are printed above)
    assert 0 < d_emul < 0.05 and np.all((got > 0) & (got < 1))
    assert d_dev <= 4 * d_emul


@pytest.mark.parametrize("decoder", ["viterbi", "argmax"])
def test_decoding_of_the_devices_own_salience(engine, clips16, decoder):
    """Masking, softmax and Viterbi of the host restatement on the salience the device fetched: identical bins on every frame, f0 within 1 ulp of
    the formula, periodicity bit-equal to the gathered salience.  Seed 17 was checked on the CPU (with the fp16-emulating restatement's
    salience of these clips at this hop): two float64 Viterbi runs that sum the softmax denominator in different orders agree on every frame;
    the test repeats that check on the device's salience, so that no frame needs to be excluded."""
    bins, f0, per, sal = run(engine, "tiny", clips16, decoder, hop=160)
    assert [len(b) for b in bins] == [1, 41, 46]
    for b, f, p, s in zip(bins, f0, per, sal):
        want, want_f0, want_per = R.decode(s, LO, HI, decoder, order="numpy")
        assert np.array_equal(want, R.decode(s, LO, HI, decoder, order="reversed")[0])
        assert np.array_equal(b, want) and (b >= LO).all() and (b < HI).all()
        assert np.all(np.abs(f - want_f0) <= np.spacing(want_f0))
        assert p.dtype == np.float32 and np.array_equal(p, want_per) and np.array_equal(p, s[np.arange(len(b)), b])
    if decoder == "viterbi":                                        # the transition holds on the device's path
        assert all(np.abs(np.diff(b)).max(initial=0) <= 11 for b in bins)


def decoder_cases():
    """name -> (salience [n, 360] float32, lo, hi): the host test's bump along a trajectory of steps up to 11 bins (followed exactly) and its jump
    of 40 bins (refused by the transition); random saliences whose best path moves -- sigmoid-like values in [0, 1] with a drifting ridge, and
    the same stretched by 6 so that the observation outweighs the transition more often --, with the mask wide open (the band clipped at bins 0 and
    359, out-of-band predecessors on both sides) and at C2 / C6."""
    b = np.arange(360)[None, :]
    bump = lambda traj: (40.0 * np.exp(-0.5 * ((b - np.asarray(traj)[:, None]) / 1.5) ** 2)).astype(np.float32)
    rng = np.random.default_rng(SEED)
    traj = [150]
    for st in rng.integers(-11, 12, size=79):
        nxt = traj[-1] + int(st)
        traj.append(nxt if 70 <= nxt < 295 else traj[-1] - int(st))
    ridge = 180 + 170 * np.sin(np.arange(300) / 30.0)
    soft = (0.25 * rng.random((300, 360)) + 0.7 * np.exp(-0.5 * ((b - ridge[:, None]) / 4.0) ** 2)).astype(np.float32)
    return {"trajectory": (bump(traj), LO, HI, np.array(traj)), "jump": (bump([100] * 6 + [140] * 6), 0, 360, None),
            "soft-open": (soft, 0, 360, None), "soft-c2c6": (soft, LO, HI, None), "sharp-open": (6 * soft, 0, 360, None),
            "one-frame": (soft[:1], 5, 17, None)}


@pytest.mark.parametrize("case", ["trajectory", "jump", "soft-open", "soft-c2c6", "sharp-open", "one-frame"])
def test_device_decoder_on_given_saliences(engine, case):
    """pce_selftest_crepe_decode (the decoding of pce_crepe_run) against the host restatement: identical bins.  Checked on the CPU for these seeded
    cases, and asserted here: the host Viterbi gives the same path whichever way it sums the softmax denominator."""
    sal, lo, hi, traj = decoder_cases()[case]
    for decoder in ("viterbi", "argmax"):
        want, want_f0, want_per = R.decode(sal, lo, hi, decoder)
        assert np.array_equal(want, R.decode(sal, lo, hi, decoder, order="reversed")[0])
        bins, f0, per = engine.selftest_crepe_decode(sal, lo, hi, decoder)
        assert np.array_equal(bins, want) and np.array_equal(per, want_per) and np.all(np.abs(f0 - want_f0) <= np.spacing(want_f0))
        if traj is not None:
            assert np.array_equal(bins, traj)
        if case == "jump" and decoder == "viterbi":
            assert np.abs(np.diff(bins)).max() <= 11 and bins[0] == 100 and bins[-1] == 140
        if case in ("soft-c2c6", "sharp-open") and decoder == "viterbi":      # (soft-open: with bins 0 / 359 unmasked the path sits at an edge state,
            # whose row of the transition is normalised over fewer entries -- the restatement's answer, and the device's)
            assert len(set(bins.tolist())) > 20                     # the path does move


@pytest.mark.parametrize("capacity,chunk", [("tiny", 16), ("full", 3)])
def test_chunk_and_batch_independence(engine, clips16, capacity, chunk):
    """frames_per_chunk = 16 (tiny: 37 frames in three chunks that cut through clips) / 3 (full) against one chunk, and every clip alone against
    the batch of three: bins, f0, periodicity and salience bit-identical."""
    whole = run(engine, capacity, clips16)
    cut = run(engine, capacity, clips16, frames_per_chunk=chunk)
    for a, b in zip(whole, cut):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for i, c in enumerate(clips16):
        alone = run(engine, capacity, [c])
        assert all(np.array_equal(whole[k][i], alone[k][0]) for k in range(4))
    am = run(engine, capacity, clips16, "argmax"), run(engine, capacity, clips16, "argmax", frames_per_chunk=chunk)
    assert all(np.array_equal(x, y) for a, b in zip(*am) for x, y in zip(a, b))


def test_product_path_rmse(engine):
    """compute_f0_rmse_batch(f0="crepe") = rmse_from_path on the contours the engine returns, NaN where nothing is voiced."""
    w = weights("tiny")
    eps = [(_tone_noise(9000, 16000, 11), _tone_noise(8000, 16000, 12)), (_tone_noise(12000, 16000, 13), _tone_noise(12500, 16000, 14))]
    got = EV.compute_f0_rmse_batch(engine, eps, 16000, hop_length=160, f0="crepe", crepe_weights=w)
    contours = EV.extract_f0_torchcrepe_batch(engine, [y for ep in eps for y in ep], 16000, 160, model="tiny", weights=w)
    assert [len(c) for c in contours] == [57, 51, 76, 79]
    for k, g in enumerate(got):
        lr, ls = (np.log(c[~np.isnan(c)]) for c in contours[2 * k:2 * k + 2])
        assert lr.size and ls.size and np.isfinite(g)
        assert g == EV.rmse_from_path(lr, ls, EV.fastdtw(lr, ls, 25, engine)[1])
    assert g == EV.compute_f0_rmse(engine, *eps[1], 16000, hop_length=160, f0="crepe", crepe_weights=w)
    assert all(np.isnan(v) for v in EV.compute_f0_rmse_batch(engine, eps, 16000, hop_length=160, f0="crepe", crepe_weights=w, crepe_threshold=1.1))
    # a 44.1 kHz recording: resampled by the engine, hop 512 -> 185
    f0 = EV.extract_f0_torchcrepe(_tone_noise(20000, 44100, 3), 44100, model="tiny", engine=engine, weights=w)
    assert len(f0) == 1 + 7257 // 185 and engine.rate == 16000


def test_errors(engine, clips16):
    with ProsodyEngine(0) as fresh:
        fresh.upload(clips16, 16000)
        with pytest.raises(PceError, match="pce_crepe_load"):
            fresh.crepe(160, EV.C2_HZ, EV.C6_HZ)
        c_out, flat = weights("tiny")
        with pytest.raises(PceError, match="floats"):
            fresh.crepe_load(c_out, flat[:-1])
        with pytest.raises(PceError):
            fresh.crepe_load((100, 16, 16, 16, 32, 64), flat)
        fresh.crepe_load(c_out, flat)
        fresh.upload(clips16, 22050)
        with pytest.raises(PceError, match="16000"):
            fresh.crepe(160, EV.C2_HZ, EV.C6_HZ)
        with pytest.raises(ValueError):
            fresh.crepe(160, EV.C2_HZ, EV.C6_HZ, decoder="weighted_argmax")
        fresh.upload(clips16, 16000)
        assert [len(b) for b in fresh.crepe(160, EV.C2_HZ, EV.C6_HZ)[0]] == [1, 41, 46]
