"""tests/decode_rules_restatement.py, which tests/test_gpu_decode_rules.py compares k_decode_rules and k_step_advance against, pinned on the host:
its filters to oracle/whisper_oracle.py's apply_decoding_rules (torch), its softmax pieces to torch, its generator to integers worked out by hand,
its loop to the host-driven loop of Aligners/decoding.py -- and the share of the GPU test's sampling inputs that its error model excuses."""
import numpy as np
import torch

from oracle import whisper_oracle as WO
from prosody_control_french_tts_amd.Aligners import decoding as DEC
from tests import decode_rules_restatement as DR
from tests import test_gpu_decode_rules as G


def _random_state(rng):
    V = int(rng.integers(24, 90))
    n_ts = int(rng.integers(1, V // 3))
    ts = V - n_ts
    eot = int(rng.integers(2, ts - 2))
    rules = dict(eot=eot, timestamp_begin=ts, no_timestamps=ts - 1, suppress_tokens=sorted(set(rng.integers(0, ts, 4).tolist()) - {eot}),
                 blank_tokens=[int(rng.integers(0, eot)), eot],
                 max_initial_timestamp_index=[None, 0, 2, 200][int(rng.integers(0, 4))])
    sb = int(rng.integers(1, 5))
    ns = [0, 0, 1, 2, 3, 7][int(rng.integers(0, 6))]
    tail = [int(rng.integers(ts, V)) if rng.random() < 0.45 else int(rng.integers(0, ts)) for _ in range(ns)]
    if ns and rng.random() < 0.15:
        tail[-1] = V - 1                                           # the last timestamp: nothing may follow it but itself
    tokens = [int(t) for t in rng.integers(0, V, sb)] + tail       # (timestamps in the prompt too)
    logits = (rng.standard_normal(V) * 3).astype(np.float32)
    if rng.random() < 0.1:
        logits[ts:] += 6.0                                        # heavy timestamps: the mass rule fires
    return V, rules, tokens, sb, logits


def test_filters_equal_the_oracle():
    rng = np.random.default_rng(2024)
    compared, fired = 0, 0
    for _ in range(500):
        V, rules, tokens, sb, logits = _random_state(rng)
        mask = DEC.vocab_mask(V, rules["suppress_tokens"], rules["blank_tokens"], rules["no_timestamps"])
        got, margin = DR.filtered(logits, tokens, sb, rules["eot"], rules["timestamp_begin"], mask, rules["max_initial_timestamp_index"])
        if np.isfinite(margin) and abs(margin) < 1e-3:
            continue                                               # (the oracle decides the mass rule in fp32: not at the threshold)
        want = WO.apply_decoding_rules(logits, tokens, sb, rules)
        assert got.dtype == np.float64 and np.array_equal(got.astype(np.float32), want), (V, rules, tokens, sb)
        compared += 1
        fired += bool(np.isfinite(margin) and margin > 0 and np.isfinite(logits[:rules["timestamp_begin"]]).any())
    assert compared >= 300 and fired >= 20


def test_choice_probe_and_log_softmax_equal_torch():
    rng = np.random.default_rng(5)
    for _ in range(50):
        x = rng.standard_normal(40) * 4
        x[rng.random(40) < 0.3] = -np.inf
        x[7] = 1.0
        t = torch.from_numpy(x)
        i, lp = DR.choose(x, [1, 2], eot=39)
        assert i == int(torch.argmax(t)) and abs(lp - float(torch.log_softmax(t, -1)[i])) < 1e-12
        raw = rng.standard_normal(40) * 4
        assert abs(DR.probe(raw, 9) - float(torch.softmax(torch.from_numpy(raw), -1)[9])) < 1e-15
    tie = np.array([-np.inf, 2.0, 5.0, 5.0, 1.0])
    assert DR.choose(tie, [0], eot=4)[0] == 2                      # first maximum
    assert DR.choose(tie, [0, 4], eot=4) == (4, 0.0)               # once end-of-text, always end-of-text, nothing added to sum_logprobs
    assert DR.choose(np.full(5, -np.inf), [0], eot=4) == (0, 0.0)


def test_uniforms():
    # by hand: seed 0, counter 0 -> the first finaliser maps 0 to 0, the second is splitmix64's well-known first output for seed 0,
    # 0xE220A8397B1DCDAF; its top 23 bits are 7409748
    assert 0xE220A8397B1DCDAF >> 41 == 7409748
    assert DR.uniforms(0, 0, 0, [0])[0] == (7409748 + 0.5) / 8388608.0
    # a general counter, worked out with 64-bit integers outside this module: seed 7 << 32 | 12345, key -3, position 17, id 51864 -> 3270265
    assert DR.uniforms(12345 + (7 << 32), -3, 17, [51864])[0] == (3270265 + 0.5) / 8388608.0
    assert DR.uniforms(1, 0, 0, [1])[0] == (3088597 + 0.5) / 8388608.0
    for seed, key, pos in ((0, 0, 0), (2 ** 40 + 6, -(1 << 30), 447), (99, 2 ** 31 - 1, 3)):
        u = DR.uniforms_np(seed, key, pos, 52224)
        assert np.array_equal(u[::997], DR.uniforms(seed, key, pos, range(0, 52224, 997)))
        assert u.min() > 0.0 and u.max() < 1.0 and np.array_equal(u.astype(np.float32).astype(np.float64), u)      # strictly inside, exact in fp32
        assert 0.49 < u.mean() < 0.51 and len(np.unique(u)) > 52000
    # the extremes of the 23 bits stay inside (0, 1) in fp32
    assert np.float32(0.5 / 8388608.0) > 0 and np.float32((8388607 + 0.5) / 8388608.0) < 1


def test_sampling_is_a_draw_from_the_scaled_softmax():
    """the Gumbel arg-max over many keys reproduces softmax(x / T), and the reported log-probability is the unscaled one"""
    x = np.array([0.0, 1.0, -np.inf, 2.0, 0.5])
    T = 2.0
    counts = np.zeros(5)
    for key in range(4000):
        i, lp, gap, p, g = DR.sample(x, [1, 2, 3], 4, T, 17, key)
        counts[i] += 1
        assert abs(lp - float(torch.log_softmax(torch.from_numpy(x), -1)[i])) < 1e-12 and gap > 0
    want = torch.softmax(torch.from_numpy(x) / T, -1).numpy()
    assert counts[2] == 0 and np.all(np.abs(counts / 4000 - want) < 4 * np.sqrt(want * (1 - want) / 4000) + 1e-9)


class _ScriptedEngine:
    """whisper_decode_step_ex from scripted logits: call s answers with the restatement's choice on logits[s]"""

    def __init__(self, vc, logits):
        self.vc, self.logits, self.step = vc, logits, 0

    def whisper_num_encoded(self):
        return self.logits.shape[1]

    def whisper_decode_step_ex(self, seqs, begins, eot, ts, mask, max_initial, temperature=0.0, seed=0, no_cache=False):
        picks = [DR.choose(DR.filtered(self.logits[self.step, i], s, int(begins[i]), eot, ts, mask, max_initial)[0], s, eot) for i, s in enumerate(seqs)]
        self.step += 1
        return np.array([p[0] for p in picks], np.int32), np.array([p[1] for p in picks]), None


def test_loop_restatement_equals_the_host_driven_loop():
    """Aligners/decoding.py's decode_batch, one whisper_decode_step_ex round trip per step with sequences beyond the context handed over as ended, and
    DR.loop (the device loop's table bookkeeping) give the same tokens and log-probabilities on the GPU test's scripted logits"""
    for n in (3, 40):
        vc, prompts, sbs, logits = G.loop_script(n)
        rules = dict(eot=vc.eot, timestamp_begin=vc.ts, no_timestamps=vc.ts - 1, max_initial_timestamp_index=1,
                     suppress_tokens=[int(v) for v in np.flatnonzero(vc.mask & 1) if v != vc.ts - 1], blank_tokens=[int(v) for v in np.flatnonzero(vc.mask & 2)])
        assert np.array_equal(DEC.vocab_mask(vc.V, rules["suppress_tokens"], rules["blank_tokens"], rules["no_timestamps"]), vc.mask)
        toks, lps, sums = DEC.decode_batch(_ScriptedEngine(vc, logits), vc.V, prompts, sbs, rules, G.LOOP_STEPS, device_loop=False, n_text_ctx=G.LOOP_CAP)
        want, _ = G.loop_want(vc, prompts, sbs, logits, G.LOOP_STEPS, G.LOOP_STEPS)
        capped = 0
        for i in range(n):
            new = want["out_tok"][i]
            cut = new.index(vc.eot) if vc.eot in new else len(new)
            assert toks[i] == new[:cut] and lps[i] == want["out_lp"][i][:cut], i
            assert abs(sums[i] - sum(want["out_lp"][i][:cut + (1 if vc.eot in new else 0)])) < 1e-12
            capped += want["len"][i] == G.LOOP_CAP
        assert capped >= 1 and any(vc.eot in t for t in want["out_tok"]) and any(vc.eot not in t for t in want["out_tok"])


def test_the_error_model_excuses_few_of_the_sampling_inputs():
    """at most 1 % of the GPU test's draws may be excused: its inputs, on the CPU, stay far inside (no draw is, at these seeds)"""
    for V in G.VOCABS:
        seeds = G.SAMPLE_SEEDS if V < 2000 else G.SAMPLE_SEEDS[:1]  # (one seed of the four at the large vocabularies: the reference costs 5 ms a row)
        for T in G.TEMPS:
            margins = np.array([w[3] for seed in seeds for w in G.sampling_want(V, T, seed)])
            assert margins.size == 64 * len(seeds) and np.mean(margins <= 0.0) <= 0.01, (V, T, float(np.mean(margins <= 0.0)))
            assert np.median(margins) > 0.3                       # (an Exp(1)-like gap: median log 2)
