"""The loudness kernels of csrc/pce_lufs.hip stage by stage against tests/lufs_restatement.py (long double), through pce_lufs_run and
pce_lufs_fetch_stages.  Every slice of every batch of tests/lufs_cases.py, every element of every stage, nothing left out:
  * the chunk and block tables EQUAL the restatement's plan; a slice's chunks tile [0, last bound) and every block's [c0, c1) covers exactly its [l, u);
    first_chunk / first_block / status / the peak divided by EQUAL; the coefficients are pyloudnorm's design to the last place or two of the host's libm;
  * the power table within its bound of the long-double powers, and EQUAL to transition_powers' float64 arithmetic restated in numpy;
  * pass 1: state_end of every chunk within the cascade bound of the long-double zero-state run;
  * the scan: state_init[0] == 0; every later begin state within its step's bound of A^len state_init[c] + state_end[c] formed from the device's own
    values -- inside a group, across a group border, across the 1024-chunk carry;
  * pass 2: every chunk's energy within the cascade bound of the long-double run from the device's own begin state;
  * whole slice: every chunk's and every block's energy against the long-double filter run over pieces of 250 samples (not the device's chunks), within the
    bound accumulated along the slice;
  * the gate: z EQUAL bit for bit to inv_norm x (the device's chunk energies added in chunk order); both gated sets decided in long double from the
    device's z, no block within 1e-6 LU of a threshold it is compared with (asserted; the allowance is below 1e-9); the final value within
    lufs_bound of -0.691 + 10 log10(mean), -inf for the slice of zeros, NaN for slices without a block.
Edges, each counted and asserted to occur (WANTS of tests/lufs_cases.py): the eight residues of the slice begin in the resident
buffer behind clips of odd length; a slice that begins before its clip, one that ends past it, one wholly outside it (over the next clip's samples: zeros by
the mask, peak 0 -> 1, -inf), one that ends at the end of a resident buffer whose size is no multiple of 8; empty and too-short slices between live ones in
a run of 20; a chunk of length 1; 13, 16 and 17 chunks; 1024 and 1025 chunks at 44.1 and 48 kHz; 64 and 65 gating blocks; exactly one block and one
sample less at 8000, 11 025, 16 000, 22 050, 44 100 and 48 000 Hz; a 44 100 Hz meter on 16 000 Hz data; blocks dropped by the absolute gate, by the relative
gate, by both.  ``lufs`` alone and ``lufs`` after ``energy_run`` of the same slices (which reuses its peaks) return the same bits and the same stages.

MEASURED (MI355X; worst |got - want| / bound over every element of every slice of every batch; 46 live slices, 7102 chunks, 487 blocks):
  table 0.329   pass1 0.236   scan_inside 0.372   scan_group 0.0108   scan_carry 0.00052   pass2 0.293   chunk 0.0029   block 2.8e-6   lufs 0.147
The tables, first_chunk / first_block, the statuses and the peaks equal the restatement's in every slice, z equals the float64 sums bit for bit in every
block, and the power table equals transition_powers' arithmetic bit for bit at all six rates.  Block energies lie within 1.7e-12 relative of the long-double
filter (44.1 / 48 kHz, 1025 chunks; 4.7e-14 at 16 kHz).  No kernel had to change.
The device's log10: the worst |device - long double| of the final value, with the device's own mean reproduced bit for bit (lane sums, butterfly, division),
is 1.554 ulps of log10's result (the 44.1 kHz meter on 16 kHz data); that figure includes the product by 10 and the sum with -0.691, which alone reach
1.55 with numpy's log10 in the emulation.  EPS_LOG10_MEASURED = 1.56, EPS_LOG10 = 4 x 1.56 = 6.24 ulps; the test asserts that no case exceeds 1.56.
"""
import numpy as np
import pytest

from tests import lufs_cases as K
from tests import lufs_restatement as R

pytestmark = pytest.mark.gpu

BATCHES = K.batches()


def run(engine, batch, after_energy=False):
    from prosody_control_french_tts_amd import engine as E
    engine.upload(batch["clips"], batch["rate"])
    engine.lufs_set_meter_rate(batch["meter"])
    try:
        sl = E.make_slices(*(np.array(v) for v in zip(*batch["slices"])))
        if after_energy:
            engine.energy_run(sl)
        lufs, status = engine.lufs(sl)
        return engine.lufs_fetch_stages(), lufs, status
    finally:
        engine.lufs_set_meter_rate(0)


def test_fetch_stages_before_a_run_is_refused(engine):
    import prosody_control_french_tts_amd as P
    engine.upload([np.zeros(8000, np.int16)], 16000)
    with pytest.raises(P.PceError, match="before pce_lufs_run"):
        engine.lufs_fetch_stages()


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_every_stage_of_every_slice(engine, name):
    batch = BATCHES[name]
    stages, lufs, status = run(engine, batch)
    worst, cnt, fails = K.check_batch(batch, stages, lufs, status)
    print("lufs-stages", name, {k: float(f"{v:.3g}") for k, v in worst.items()}, {k: (sorted(v) if isinstance(v, set) else v) for k, v in cnt.items()})
    assert not fails, fails[:10]
    assert K.wanted(name, cnt), cnt
    assert cnt["margin"] >= 1e-6 and R.level_allowance(65) < 1e-9
    assert cnt["log10_ulps"] <= R.EPS_LOG10_MEASURED, "the device's log10 is further from the long double's than the figure EPS_LOG10 was taken from"


def test_peaks_reused_from_energy_run_give_the_same_bits(engine):
    batch = BATCHES["addresses_16k"]
    a, la, sa = run(engine, batch)
    b, lb, sb = run(engine, batch, after_energy=True)
    assert np.array_equal(sa, sb) and np.array_equal(la.view(np.uint64), lb.view(np.uint64))
    for k in ("coef", "apow", "chunks", "slices", "blocks"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert set(a["slices"]["peak"].tolist()) >= {1, 32767, 32768, 12345}
