"""tests/resample_restatement.py on the CPU: the long-double reference is the spec oracle.resample_int16 states with scipy, on the clips
tests/test_gpu_resample.py resamples on the device, and none of their samples lies near a rounding tie.

For every ratio the product takes (44 100, 48 000, 24 000, 22 050 and 8 000 -> 16 000; 16 000 -> 22 050 and 44 100) and every clip of the ragged batch:
output lengths are ceil(n up / down); oracle.resample_int16 (scipy's float64 upfirdn) EQUALS rint of the long-double sum, saturated, in every sample; no
exact value lies within (taps used + 1) 2^-53 sum |h x| of a half-integer (the nearest stays more than 40 000 such windows away), so the device test asserts equality
without the one-LSB exception; the full-scale square reaches both rails at every ratio.  The rational-arithmetic reference of the dyadic-tap cases agrees with the long
double one and holds half-to-even ties in both directions and both saturation limits."""
import numpy as np
import pytest

from tests import resample_restatement as RS


def _filter(rate_in, rate_out):
    from prosody_control_french_tts_amd.hostrules import resample_filter
    return resample_filter(rate_in, rate_out)


@pytest.mark.parametrize("rates", RS.RATIOS, ids=lambda r: f"{r[0]}-{r[1]}")
def test_reference_is_the_oracle_and_no_sample_is_near_a_tie(rates):
    from oracle import oracle as O
    up, down, taps, pre = _filter(*rates)
    span = -(-len(taps) // up)
    for k, x in enumerate(RS.clips(*rates, span)):
        want, near, y = RS.reference(x, up, down, taps, pre)
        assert len(want) == -(-len(x) * up // down)
        if len(x):
            assert np.array_equal(O.resample_int16(x, *rates), want), (rates, k)
        assert not near.any(), (rates, k, int(near.sum()))
        if k == 5:
            assert (want == 32767).any() and (want == -32768).any(), rates


def test_dyadic_taps_give_ties_both_ways_and_both_rails():
    x = RS.tie_clip()
    seen = set()
    for up, down, taps, pre in RS.TIES:
        want = RS.exact(x, up, down, taps, pre)
        ref, near, y = RS.reference(x, up, down, taps, pre)
        assert np.array_equal(want, ref)
        half = (y - np.floor(y)) == 0.5
        assert half.any() and near[half].all()                   # exact ties: the long double holds them exactly
        lo = np.floor(y[half]).astype(np.int64)
        seen |= {"down" if v % 2 == 0 else "up" for v in lo}       # floor even: the tie goes down to it; odd: up
        seen |= {"top"} if (y >= 32767.5).any() else set()
        seen |= {"bottom"} if (y <= -32768.5).any() else set()
        seen |= {"top-tie"} if (y == 32767.5).any() else set()
        seen |= {"bottom-tie"} if (y == -32767.5).any() else set()
    assert seen == {"down", "up", "top", "bottom", "top-tie", "bottom-tie"}, seen
