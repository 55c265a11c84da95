"""k_resample (csrc/pce_resample.hip) at every ratio the product takes, against tests/resample_restatement.py (long double), through
``ProsodyEngine.resample``; and with caller-made dyadic taps, where every sum is exact, bit for bit against rational arithmetic.

Ratios: 44 100, 48 000, 24 000, 22 050 and 8 000 -> 16 000; 16 000 -> 22 050 (evaluate_voice) and 44 100.  One ragged batch per ratio: clips of 0 samples and of 1
sample, one sample shorter and one longer than the filter's span len(taps) / up, 0.3 s of seeded noise, a full-scale +-32767 square whose overshoot
saturates at both rails (asserted: some outputs are 32767 and some -32768).  Output lengths are ceil(n up / down).  Every output sample EQUALS rint of
the long-double sum, saturated: tests/test_resample_host.py shows that no exact value of these clips lies within (taps used + 1) 2^-53 sum |h x| of a
half-integer, which is asserted here again, so the one-LSB exception of a near tie is never taken (the cap of 1e-4 of a clip's samples is not needed).
Exact ties: taps [0.5, 0.5] at 1/1, [0.25, 0.5, 0.25] at 1/2, [0.5, 1, 0.5] at 2/1 and [1.5, 1] at 1/1 on small integers and the int16 limits: half to even in both
directions, 32767.5 -> 32767 and -32768.5 -> -32768 by saturation, EQUAL in every sample."""
import numpy as np
import pytest

from tests import resample_restatement as RS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("rates", RS.RATIOS, ids=lambda r: f"{r[0]}-{r[1]}")
def test_every_sample_is_the_rounded_long_double_sum(engine, rates):
    from prosody_control_french_tts_amd.hostrules import resample_filter
    up, down, taps, pre = resample_filter(*rates)
    src = RS.clips(*rates, -(-len(taps) // up))
    engine.upload(src, rates[0])
    engine.resample(rates[1])
    assert engine.rate == rates[1]
    got = engine.download()
    assert len(got) == len(src)
    for k, (x, y) in enumerate(zip(src, got)):
        want, near, _ = RS.reference(x, up, down, taps, pre)
        assert len(y) == len(want) == -(-len(x) * up // down), (k, len(y))
        assert not near.any()
        assert np.array_equal(y, want), (k, int((y != want).sum()), int(np.abs(y.astype(np.int32) - want).max()))
    assert (got[5] == 32767).any() and (got[5] == -32768).any()


@pytest.mark.parametrize("case", range(len(RS.TIES)))
def test_exact_ties_and_saturation_with_dyadic_taps(engine, case):
    up, down, taps, pre = RS.TIES[case]
    x = RS.tie_clip()
    engine.upload([x, x[:1], x[:0], x[::-1].copy()], 16000)
    engine.resample(16000 * up // down, filter=(up, down, taps, pre))
    got = engine.download()
    for src, y in zip((x, x[:1], x[:0], x[::-1]), got):
        assert np.array_equal(y, RS.exact(src, up, down, taps, pre))
