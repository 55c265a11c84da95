"""Known answers of the float64 attention restatement (tests/attention_restatement.py) the GPU attention tests compare against."""
import numpy as np
import torch

from tests import attention_restatement as AR


def _rand(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape)


def test_equal_scores_give_the_mean_of_v():
    q, v = _rand(0, 3, 64), _rand(1, 11, 64)
    k = np.tile(_rand(2, 1, 64), (11, 1))                    # the same key eleven times: equal scores whatever the query
    out, A = AR.attention(q, k, v)
    assert np.allclose(out, np.tile(v.mean(axis=0), (3, 1)), rtol=0, atol=1e-15)
    assert np.allclose(A, np.tile(np.abs(v).mean(axis=0), (3, 1)), rtol=0, atol=1e-15)
    out0, _ = AR.attention(np.zeros((2, 64)), _rand(3, 11, 64), v)      # a zero query: every score is 0
    assert np.allclose(out0, np.tile(v.mean(axis=0), (2, 1)), rtol=0, atol=1e-15)


def test_a_key_80_above_the_rest_gives_its_row():
    q = np.zeros((1, 64)); q[0, 0] = 8.0                     # score of key t = k[t, 0]
    k = np.zeros((9, 64)); k[:, 0] = np.arange(9) * 0.25; k[5, 0] = 2.0 + 80.0
    v = _rand(4, 9, 64)
    out, A = AR.attention(q, k, v)
    assert np.max(np.abs(out[0] - v[5])) <= 1e-30                  # (the others weigh e^-80 = 1.8e-35 each)
    assert np.max(np.abs(A[0] - np.abs(v[5]))) <= 1e-30


def test_one_key_returns_its_value():
    q, k, v = _rand(5, 4, 64), _rand(6, 1, 64), _rand(7, 1, 64)
    out, A = AR.attention(q, k, v)
    assert np.array_equal(out, np.tile(v, (4, 1))) and np.array_equal(A, np.tile(np.abs(v), (4, 1)))
    out, _ = AR.attention(q, _rand(8, 5, 64), np.concatenate([v, _rand(9, 4, 64)]), n_keys=1)       # the key count cuts the key axis
    assert np.array_equal(out, np.tile(v, (4, 1)))


def test_causal_mask_three_by_three_by_hand():
    q = np.zeros((3, 64)); q[:, 0] = 8.0                     # score of (query i, key t) = k[t, 0]
    k = np.zeros((3, 64)); k[:, 0] = [0.0, np.log(2.0), np.log(5.0)]
    v = np.zeros((3, 64)); v[:, 0] = [1.0, -1.0, 3.0]; v[:, 1] = [1.0, 10.0, 100.0]
    out, A = AR.attention(q, k, v, causal=True)
    # weights: row 0 = [1]; row 1 = [1, 2] / 3; row 2 = [1, 2, 5] / 8
    want0 = [1.0, (1.0 - 2.0) / 3.0, (1.0 - 2.0 + 15.0) / 8.0]
    wantA = [1.0, (1.0 + 2.0) / 3.0, (1.0 + 2.0 + 15.0) / 8.0]
    want1 = [1.0, 21.0 / 3.0, 521.0 / 8.0]
    assert np.allclose(out[:, 0], want0, rtol=0, atol=1e-15) and np.allclose(out[:, 1], want1, rtol=1e-15, atol=0)
    assert np.allclose(A[:, 0], wantA, rtol=0, atol=1e-15) and np.all(out[:, 2:] == 0)
    p, mag = AR.weights(q, k, causal=True)
    assert np.array_equal(p == 0, np.triu(np.ones((3, 3), dtype=bool), 1))
    assert np.allclose(mag, np.tile(np.abs(k[:, 0]), (3, 1)), rtol=1e-15, atol=0)
    full, _ = AR.attention(q, k, v)                           # without the mask every row is row 2
    assert np.allclose(full[:, 0], want0[2], rtol=0, atol=1e-15)


def test_agrees_with_torch_softmax_in_float64():
    H, Q, K = 5, 13, 37
    q, k, v = _rand(10, H, Q, 64) * 1.5, _rand(11, H, K, 64) * 1.5, _rand(12, H, K, 64)
    for causal in (False, True):
        tq, tk, tv = (torch.from_numpy(x) for x in (q, k, v))
        s = tq @ tk.transpose(-1, -2) / 8.0
        if causal:
            s = s + torch.full((Q, K), float("-inf"), dtype=torch.float64).triu(1)
        p = torch.softmax(s, dim=-1)
        out, A = AR.attention(q, k, v, causal=causal)
        assert np.max(np.abs(out - (p @ tv).numpy())) <= 1e-14
        assert np.max(np.abs(A - (p @ tv.abs()).numpy())) <= 1e-14
    flat = AR.merge_heads(q)
    assert flat.shape == (Q, H * 64) and np.array_equal(AR.split_heads(flat, H), q)
