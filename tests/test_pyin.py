"""pYIN restatement (oracle/pyin_oracle.py, third party behaviour restated: parity unpinned) on analytic cases, and
the host plan tables of the product against the restatement's dense matrices."""
import numpy as np

from oracle import pyin_oracle as PO
from prosody_control_french_tts_amd.visualisation import acoustic_analysis as AA


def test_known_answers():
    sr = 16000
    t = np.arange(int(0.8 * sr)) / sr
    for f in (110.0, 220.0, 523.25):
        y = (0.4 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 2 * f * t)).astype(np.float32)
        f0, voiced, vp = PO.pyin(y, sr)
        mid = slice(8, len(f0) - 8)
        assert voiced[mid].all() and np.all(vp[mid] > 0.9)
        assert np.max(np.abs(12 * np.log2(f0[mid] / f))) <= 0.06            # within half a 0.1-semitone bin
    f0, voiced, vp = PO.pyin(np.zeros(sr // 2, np.float32), sr)
    assert not voiced.any() and np.all(np.isnan(f0)) and np.all(vp == 0)
    rng = np.random.default_rng(0)
    f0, voiced, vp = PO.pyin((0.1 * rng.standard_normal(sr // 2)).astype(np.float32), sr)
    assert voiced.mean() < 0.2
    assert len(f0) == 1 + (sr // 2) // 256


def test_fft_route_and_exact_difference_function_agree():
    sr = 16000
    rng = np.random.default_rng(1)
    t = np.arange(int(0.6 * sr)) / sr
    y = (0.3 * np.sin(2 * np.pi * (180 + 40 * t) * t) + 0.02 * rng.standard_normal(len(t))).astype(np.float32)
    y = (np.round(y * 32768) / 32768).astype(np.float32)                    # int16-valued samples, as librosa.load gives for 16-bit WAVs
    a = PO.pyin(y, sr, want_intermediate=True)
    b = PO.pyin(y, sr, want_intermediate=True, exact=True)
    assert np.max(np.abs(a[3]["yin"] - b[3]["yin"])) < 1e-3                 # float32 FFT noise around the exact values
    same = (a[0] == b[0]) | (np.isnan(a[0]) & np.isnan(b[0]))
    assert same.mean() >= 0.97 and np.max(np.abs(a[2] - b[2])) < 0.1


def test_host_plan_tables_equal_the_dense_matrices():
    for sr in (16000, 44100):
        plan, tables, freqs = AA.pyin_plan(sr)
        nb, W = plan.n_pitch_bins, plan.trans_width
        half = W // 2
        assert nb == 608 and plan.min_period == int(np.floor(sr / 2000.0)) and W == (71 if sr == 16000 else 31)
        T = PO.transition_local_triangle(nb, W)
        full = np.log(np.kron(np.array([[0.99, 0.01], [0.01, 0.99]]), T) + PO.TINY64)
        o = 100 + 100 + 101 + 2 * (AA.MAX_TROUGHS + 1)
        o += o % 2
        pairs = tables[o:].reshape(W, nb, 2); lt = pairs[:, :, 0]; ls = pairs[:, :, 1]
        for e in range(-half, half + 1):
            ks = np.arange(max(0, -e), min(nb, nb - e))
            assert np.array_equal(lt[e + half, ks], full[ks, ks + e]) and np.array_equal(ls[e + half, ks], full[ks, nb + ks + e])
        th = np.linspace(0, 1, 101)
        assert np.array_equal(tables[:100], th[1:])
        assert np.allclose(tables[100:200], np.diff(PO.beta_cdf_2_18(th)), rtol=0, atol=0)
        assert np.allclose(freqs, 60.0 * 2 ** (np.arange(nb) / 120.0))


def _clips():
    """The clips of the tests above: int16-valued, as the engine holds them."""
    sr = 16000
    rng = np.random.default_rng(1)
    t = np.arange(int(0.6 * sr)) / sr
    chirp = (0.3 * np.sin(2 * np.pi * (180 + 40 * t) * t) + 0.02 * rng.standard_normal(len(t))).astype(np.float32)
    t = np.arange(int(0.4 * sr)) / sr
    tone = (0.4 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    noise = (0.1 * np.random.default_rng(0).standard_normal(sr // 4)).astype(np.float32)
    return sr, [(np.round(y * 32768) / 32768).astype(np.float32) for y in (chirp, tone, noise, np.zeros(sr // 4, np.float32))]


def test_observation_lists_scatter_to_the_dense_matrix_and_viterbi_log_decodes_it():
    sr, clips = _clips()
    for exact in (True, False):
        for y in clips[:2] if not exact else clips:
            _, _, vp, im = PO.pyin(y, sr, want_intermediate=True, exact=exact)
            nb = im["n_pitch_bins"]
            obs, ovp, info = PO.observations(y, sr, exact=exact)
            dense = np.zeros_like(im["obs"])
            for f, (b, p) in enumerate(obs):
                assert len(set(b.tolist())) == len(b) and np.all((b >= 0) & (b < nb)) and np.all(p != 0)
                dense[b, f] = p
            dense[nb:, :] = (1 - ovp[None, :]) / nb
            assert np.array_equal(ovp, vp) and np.array_equal(dense, im["obs"])
            # a subset of the frames is those frames of the whole
            sel = [0, len(obs) // 2, len(obs) - 1]
            sub, svp, _ = PO.observations(y, sr, exact=exact, frames=sel)
            for i, f in enumerate(sel):
                assert np.array_equal(sub[i][0], obs[f][0]) and np.array_equal(sub[i][1], obs[f][1]) and svp[i] == ovp[f]
            if exact:
                T = np.kron(np.array([[0.99, 0.01], [0.01, 0.99]]), im["trans"])
                states = PO.viterbi_log(np.log(im["obs"].T + PO.TINY64), np.log(T + PO.TINY64), np.log(np.ones(2 * nb) / (2 * nb) + PO.TINY64))
                assert np.array_equal(states, im["states"])


def test_out_of_band_predecessors_tie_on_the_rounded_sum():
    """Two probabilities an ulp or so apart in frame 0, a target beyond the band of both in frame 1: V[100] < V[101], but both
    V + log(tiny) round to the same sum, and the dense argmax takes the first.  (Also on the other side of the target.)"""
    nb, width = 608, 71
    T = np.kron(np.array([[0.99, 0.01], [0.01, 0.99]]), PO.transition_local_triangle(nb, width))
    p_init = np.ones(2 * nb) / (2 * nb)
    for lo, target in ((100, 300), (500, 300)):
        prob = np.zeros((2 * nb, 2))
        prob[lo, 0] = 0.5; prob[lo + 1, 0] = 0.5 * (1 + 1e-15); prob[target, 1] = 1.0
        assert prob[lo + 1, 0] > prob[lo, 0]
        v = np.log(prob[:, 0] + PO.TINY64)
        assert v[lo + 1] > v[lo] and v[lo + 1] + np.log(PO.TINY64) == v[lo] + np.log(PO.TINY64)
        assert PO.viterbi(prob, T, p_init).tolist() == [lo, target]
