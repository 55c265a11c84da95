"""tests/lufs_restatement.py on the CPU: the long-double restatement is pyloudnorm's loudness, its plan is the host plan of csrc/pce_lufs.hip, and the stage
bounds are neither too tight for the kernels' arithmetic nor so wide that a defect fits (tests/test_gpu_lufs_stages.py applies the same bounds, through the
same loop, to what the device left).

Agreement.  On the synthetic clips below the restatement (float64 coefficients, long-double filter and sums) lies within 2.5e-12 LU of
oracle.lufs_numpy and of oracle.lufs_c; 1e-10 is asserted.

Non-vacuity.  R.emulate restates the four kernels in float64 numpy, operation for operation (chunked, the same table, the same three scan levels; the scan's
fmas through the long double), and takes a defect on request.  The faithful emulation's worst |got - want| / bound over every batch of tests/lufs_cases.py:

    stage          worst    what it is held against
    table          0.329    the long-double powers of A (44.1 kHz; the table also EQUALS transition_powers' arithmetic restated in numpy)
    pass1          0.236    the long-double zero-state run of every chunk
    scan_inside    0.359    one lu_matvec from the emulation's own state_init, state_end and table entry
    scan_group     0.0108   the long-double chain over the previous group (the bound carries the filter's growth once more: loose)
    scan_carry     0.00052  the same across chunk 1024
    pass2          0.305    the long-double run from the emulation's own begin state
    chunk          0.0029   the long-double filter over pieces of 250 samples, bound accumulated along the slice
    block          2.8e-6   the same per gating block
    lufs           0.140    -0.691 + 10 log10 of the long-double mean (numpy's log10 standing in for the device's)

The whole-slice bounds (chunk, block) are a priori worst cases over up to 1025 chunks of a filter whose state responses reach 74 (48 kHz): they allow
about 1e-6 of a block's energy at 44.1 / 48 kHz, where the emulation is off by 1e-12.  The sharp checks are the stage checks: every defect below leaves one
of them by orders of magnitude (test_every_defect_leaves_a_bound asserts it):

    defect                                   stage that fails                  ratio
    a sample dropped at a chunk border       pass1 (pass2, chunk, block too)   7.9e12
    the clip-edge mask off by one sample     pass1, pass2                      6.1e6, 2.1e8   (a slice that ends past its clip, over the next clip's samples)
    a group's begin state taken as zero      scan_group                        7.1e13
    the carry into chunk 1024 dropped        scan_carry                        3.5e13
    table entry 200 replaced by entry 199    table                             2.0e13         (and the bit comparison with transition_powers' arithmetic)
    a block summed over [c0, c1 + 1)         z, bit for bit                    not equal
    > for >= at the absolute gate            the final value                   2.84 LU        (test_strict_comparison_at_the_absolute_gate_is_seen)

Every block of every batch lies at least 1.8 LU from each threshold it is compared with (asserted: 1e-6; the float64 levels can be off the long double's
by less than 1e-9, R.level_allowance)."""
import numpy as np
import pytest

from tests import lufs_cases as K
from tests import lufs_restatement as R

BATCHES = K.batches()
WORST = {}


def test_long_double_is_wider_than_float64():
    assert np.finfo(R.LD).eps < 2.0 ** -60, "np.longdouble is no wider than float64 on this host: the restatement has no head room"


def test_restatement_agrees_with_the_oracles():
    from oracle import oracle as O
    worst = 0.0
    for rate, kind, n in ((8000, "tone20", 9000), (11025, "min", 12001), (16000, "square", 20000), (16000, "gate_both", 40000), (22050, "tone20", 30001),
                          (44100, "gate_rel", 60000), (48000, "tone20", 50001), (48000, "const", 24000)):
        clip = K.signal(kind, n, rate, 3).astype(float)
        got, _ = R.lufs_restated(clip, rate)
        for want in (O.lufs_numpy(clip, rate), O.lufs_c(clip, rate)):
            d = abs(got - want) if np.isfinite(want) else (0.0 if got == want else np.inf)
            worst = max(worst, d)
            assert d < 1e-10, (rate, kind, got, want)
    print("lufs-host oracle agreement", worst)
    with pytest.raises(ValueError):
        R.lufs_restated(np.ones(3199), 8000)


def test_rows_of_250_equal_the_sample_loop():
    for rate in (8000, 48000):
        x = K.signal("tone20", 1777, rate, 9) / 32768.0
        coef = R.kweight_float64(rate)
        a, b = R.sequential(coef, x), R.sequential_plain(coef, x)
        # both carry long-double roundings only; a state's rounding reaches u through the filter's growth G twice over (74 at 48 kHz: 3e-16 of u^2)
        G = float(R.growth(coef).max())
        assert np.max(np.abs(a - b)) < 16 * G * G * 2.0 ** -64 * np.max(b)


def test_plan_gives_the_listed_lengths():
    want = {(16000, 7425): (31, 2, 1), (8000, 3200): (13, 1, 128), (8000, 3601): (16, 2, None), (8000, 3713): (17, 2, None), (44100, 250801): (1024, 54, 1),
            (44100, 251057): (1025, 54, 1), (48000, 258497): (1024, 51, 1), (48000, 258753): (1025, 51, 1), (16000, 106401): (466, 64, None),
            (16000, 108001): (473, 65, None)}
    for (rate, ns), (nc, nb, lmin) in want.items():
        p = R.plan(ns, rate)
        assert (len(p["rel"]), len(p["c0"])) == (nc, nb) and (lmin is None or p["len"].min() == lmin), (rate, ns)
    for rate in (8000, 11025, 16000, 22050, 44100, 48000):
        n1 = K.one_block(rate)
        assert len(R.plan(n1, rate)["c0"]) == 1 and R.plan(n1 - 1, rate)["status"] == R.TOO_SHORT and R.plan(0, rate)["status"] == R.EMPTY
    p = R.plan(11025, 11025)                                  # block bounds on half samples
    assert p["lo"][:3] == [0, 1102, 2205] and p["up"][:2] == [4410, 5512]


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_the_emulation_passes_every_bound(name):
    batch = BATCHES[name]
    stages, lufs, status = K.emulate_batch(batch)
    worst, cnt, fails = K.check_batch(batch, stages, lufs, status)
    print("lufs-host", name, {k: float(f"{v:.3g}") for k, v in worst.items()}, {k: v for k, v in cnt.items() if k != "residues"})
    assert not fails, fails
    assert K.wanted(name, cnt), cnt
    assert R.level_allowance(65) < 1e-9 and (cnt["margin"] >= 1e-6)
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)


DEFECTS = {"border_sample": ("short_8000", 2, "pass1"), "clip_mask": ("addresses_16k", 10, "pass1"), "group_zero": ("short_22050", 2, "scan_group"),
           "carry_dropped": ("long_44100", 1, "scan_carry"), "table_entry": ("short_8000", None, "power table"), "block_plus_one": ("short_8000", 2, "z_equal")}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_every_defect_leaves_a_bound(defect):
    name, only, stage = DEFECTS[defect]
    batch = dict(BATCHES[name])
    if only is not None:                                      # the one slice is enough
        batch["slices"] = [batch["slices"][only]]; only = 0
    stages, lufs, status = K.emulate_batch(batch, defect, only)
    worst, cnt, fails = K.check_batch(batch, stages, lufs, status)
    print("lufs-host defect", defect, fails[:3], {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert any(stage in f for f in fails), (defect, fails)
    if stage in worst:
        assert worst[stage] > 100.0


def test_strict_comparison_at_the_absolute_gate_is_seen():
    """A block whose float64 level is -70.0 exactly counts for the first mean (>=) and not for the second (>).  With one loud block, one 14 dB under it and
    one on the gate, the relative threshold lies under the middle block with the gate block counted (-15.29) and over it without (-13.53)."""
    z = np.float64(10.0 ** -6.9309)
    edge = None
    for _ in range(200):
        if -0.691 + 10.0 * np.log10(z) == -70.0:
            edge = z; break
        z = np.nextafter(z, 1.0 if -0.691 + 10.0 * np.log10(z) < -70.0 else 0.0)
    assert edge is not None
    zs = np.array([1.0, edge, 10.0 ** -1.4])
    want = R.gate_float64(zs)
    assert abs(R.emulate_gate(zs) - want) <= R.lufs_bound(3, want) and abs(want - (-0.691 + 10 * np.log10(0.5 * (1 + 10.0 ** -1.4)))) < 1e-12
    assert abs(R.emulate_gate(zs, "gate_strict") - want) > 1.0                # -0.691 against -3.53
    assert R.gate_ld(zs)["margin"] < 1e-12                                  # ... and the long double calls the block undecidable, as it must
