"""Whisper large-v3 / turbo shapes on the device (d = 1280, 20 heads of 64, 128 mels): the encoder-output cross-attention of a decoding step with
two 16-row tiles of heads (``k_xattn_absorbed<1280>``, 8 waves), the single-query attention kernels launched as head groups of at most 16 waves,
the 128-mel front end and encoder, and the aligner end to end from a turbo-shaped checkpoint.  Models are random-init miniatures (1-2 encoder
layers, 2-4 decoder layers, 300 tokens unless stated): no trained weights exist offline."""
import json
import logging
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import whisper_oracle as WO
from prosody_control_french_tts_amd import synth, whisper_weights as WW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, H = 1280, 20


def _fresh_engine(**env):
    """A context created with the given switches in the environment (the library reads them when a context is created)."""
    import prosody_control_french_tts_amd as P
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return P.ProsodyEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _gold():
    from tests.test_whisper_hf_crosscheck import _greedy_gold
    g, rules = _greedy_gold()
    return g["initial"].tolist(), rules


def _decode(eng, edims, tdims, We, Wd, clips, prompts, begins, sample_len, active=None, n_mels=80):
    from prosody_control_french_tts_amd.Aligners import decoding as DEC
    _, rules = _gold()
    eng.upload(clips, 16000); eng.logmel_run(n_mels)
    eng.whisper_load(edims, WW.pack(We, edims)); eng.whisper_encode_run()
    eng.whisper_decoder_load(tdims, WW.pack_decoder(Wd, tdims))
    return DEC.decode_batch(eng, tdims["n_vocab"], prompts, begins, rules, sample_len=sample_len, active=active)


def test_encoder_output_cross_attention_at_20_heads_against_a_float64_restatement(engine):
    """``k_xq_fused<1280>`` -> ``k_xattn_absorbed<1280>`` -> ``k_uv_absorb<1280>`` for one layer, against the float64 restatement and bounds of
    tests/test_gpu_whisper.py's d <= 1024 test; the bits do not depend on the workgroups per clip (4 / 2 / 1 / what the batch selects) nor on the
    batch.  Heads 16..19 -- the second row tile, where a row-tile error would sit -- are checked on their own as well."""
    engine.whisper_set_operands("fp16")
    rng = np.random.default_rng(1000 + D)
    n, k_cap = 5, 1500
    k_len = np.array([1500, 1499, 700, 33, 1], dtype=np.int32)
    resid = rng.standard_normal((n, D)).astype(np.float32) * 1.5 + 0.2
    ln_w = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32); ln_b = (0.05 * rng.standard_normal(D)).astype(np.float32)
    sc = 1.0 / np.sqrt(D)
    wq, wk, wv = (rng.standard_normal((D, D)).astype(np.float32) * sc * g for g in (1.6, 1.6, 1.0))
    bq, bv = (0.1 * rng.standard_normal(D)).astype(np.float32), (0.1 * rng.standard_normal(D)).astype(np.float32)
    E = rng.standard_normal((n, k_cap, D)).astype(np.float32)
    E[:, :, : D // 2] += rng.standard_normal((n, 1, D // 2)).astype(np.float32)
    outs = {}
    for wpc in (4, 2, 1, 0):
        outs[wpc], rq, rk, rv, rE = engine.selftest_xattn(resid, ln_w, ln_b, wq, bq, wk, wv, bv, E, k_len, H, wpc)
    for wpc in (2, 1, 0):
        assert outs[wpc].tobytes() == outs[4].tobytes(), wpc
    solo = engine.selftest_xattn(resid[:2], ln_w, ln_b, wq, bq, wk, wv, bv, E[:2], k_len[:2], H, 0)[0]
    assert solo.tobytes() == outs[4][:2].tobytes()
    r16 = lambda x: x.astype(np.float16).astype(np.float64)
    x = resid.astype(np.float64)
    mu = x.mean(axis=1, keepdims=True); var = ((x - mu) ** 2).mean(axis=1, keepdims=True)
    ln = r16((x - mu) / np.sqrt(var + 1e-5) * ln_w + ln_b)
    q = r16(ln @ rq.astype(np.float64).T + bq)
    want = np.zeros((n, D))
    for c in range(n):
        Ec = rE[c, : k_len[c]].astype(np.float64)
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            s_ = ((Ec @ rk[sl].astype(np.float64).T) @ q[c, sl]) * 0.125
            p = np.exp(s_ - s_.max()); p /= p.sum()
            want[c, sl] = rv[sl].astype(np.float64) @ (p @ Ec) + bv[sl]
    got = outs[4].astype(np.float64)
    scale = np.abs(want).max()
    err = np.abs(got - want)
    assert np.all(err <= np.abs(want) * 2.0 ** -10 + 1.0e-3 * scale), (float(err.max()), float(scale))
    assert np.sqrt(np.mean(err ** 2)) <= 4.0e-4 * scale, (float(np.sqrt(np.mean(err ** 2))), float(scale))
    hi = slice(1024, 1280)                                                        # heads 16..19
    assert np.all(err[:, hi] <= np.abs(want[:, hi]) * 2.0 ** -10 + 1.0e-3 * scale)
    assert np.sqrt(np.mean(err[:, hi] ** 2)) <= 4.0e-4 * scale
    assert np.abs(got[:, hi] - bv[hi]).max() > 0.1 * scale                         # (the heads really attend: not just the bias)


def test_free_running_decoding_at_20_heads_absorbed_against_the_kv_form_and_the_restatement():
    """At d = 1280 with 20 heads the encoder-output form now runs (it used to fall back to the K / V form without a word): one context per form,
    the same free-running loop (ragged prompts, a clip inactive from the start), checked as tests/test_gpu_whisper.py checks d <= 1024.  The two
    forms are different arithmetic, so their log-probabilities must NOT be bit-identical over the run: identical bits mean one form ran twice."""
    init, rules = _gold()
    n = 3
    edims = dict(n_mels=80, n_ctx=1500, n_state=D, n_head=H, n_layer=1)
    tdims = dict(n_vocab=300, n_text_ctx=96, n_state=D, n_head=H, n_layer=2)
    We, Wd = WW.synthetic_weights(edims, seed=177), WW.greedy_test_decoder_weights(tdims, seed=179)
    use = [synth.synth_clip(40 + i, seconds=3.0 + i) for i in range(n)]
    prompts = [[7, 11 + i, 13][: i % 3 + 1] * (i + 1) + list(init) for i in range(n)]
    begins = [len(p) for p in prompts]
    active = [i != 1 for i in range(n)]
    runs = {}
    for form in ("1", "0"):
        eng = _fresh_engine(PCE_XATTN_ABSORB=form)
        try:
            toks, lps, _ = _decode(eng, edims, tdims, We, Wd, use, prompts, begins, 12, active)
            runs[form] = (toks, lps, [eng.whisper_encode_fetch(i) for i in range(n)])
        finally:
            eng.close()
    (ta, la, encs), (tb, lb, _) = runs["1"], runs["0"]
    assert ta[1] == [] and tb[1] == []
    err = {"1": [], "0": []}
    for i in range(n):
        if not active[i]:
            continue
        agree = next((k for k, (x, y) in enumerate(zip(ta[i], tb[i])) if x != y), min(len(ta[i]), len(tb[i])))
        assert agree >= 3, (i, ta[i], tb[i])
        assert np.allclose(la[i][:agree], lb[i][:agree], atol=0.02), (i, la[i][:agree], lb[i][:agree])
        seq = list(prompts[i])
        for k in range(agree):
            logits = WO.find_alignment(seq, encs[i], Wd, tdims, 2, 0, want_internal=True)["logits"][-1]
            f = WO.apply_decoding_rules(logits, seq, begins[i], rules)
            lsm = f - (np.max(f) + np.log(np.sum(np.exp(f[np.isfinite(f)] - np.max(f)))))
            err["1"].append(abs(la[i][k] - lsm[ta[i][k]])); err["0"].append(abs(lb[i][k] - lsm[ta[i][k]]))
            seq.append(ta[i][k])
    assert max(err["1"]) <= 0.05 and max(err["0"]) <= 0.05, (max(err["1"]), max(err["0"]))
    assert np.mean(err["1"]) <= 1.25 * np.mean(err["0"]) + 1e-4, (np.mean(err["1"]), np.mean(err["0"]))
    bits = lambda l: b"".join(np.asarray(x, dtype=np.float32).tobytes() for x in l)
    assert bits(la) != bits(lb)


def test_a_clips_decoding_at_20_heads_does_not_depend_on_the_batch_size(tmp_path):
    """The same 13 recordings decoded alone and in batches of 130 / 260 (4 / 4 / 2 workgroups per clip) at d = 1280 with 20 heads: tokens and
    log-probabilities bit-identical; and the workgroups per clip forced to 4 / 2 / 1 (``PCE_XATTN_WPC``, read once per process) give one hash.
    (Not a batch of 520: at d = 1280 the ENCODER's fc2 operand of 520 clips passes 4 GiB, beyond the 32-bit offsets of the persistent GEMM, so
    its projection takes the tiled kernel -- another summation order before the decoder runs.  One workgroup per clip is the forced case here.)"""
    init, _ = _gold()
    edims = dict(n_mels=80, n_ctx=1500, n_state=D, n_head=H, n_layer=1)
    tdims = dict(n_vocab=300, n_text_ctx=96, n_state=D, n_head=H, n_layer=2)
    We, Wd = WW.synthetic_weights(edims, seed=277), WW.greedy_test_decoder_weights(tdims, seed=279)
    base = [synth.synth_clip(80 + i, seconds=1.0 + 0.25 * (i % 5)) for i in range(13)]

    def decode(n):
        eng = _fresh_engine()
        try:
            return _decode(eng, edims, tdims, We, Wd, [base[i % 13] for i in range(n)], [list(init)] * n, [len(init)] * n, 8)[:2]
        finally:
            eng.close()

    ref_t, ref_l = decode(13)
    assert len({np.asarray(x, dtype=np.float32).tobytes() for x in ref_l}) > 6
    for n in (130, 260):
        t, l = decode(n)
        for i in range(n):
            assert t[i] == ref_t[i % 13], (n, i, t[i], ref_t[i % 13])
            assert np.asarray(l[i], dtype=np.float32).tobytes() == np.asarray(ref_l[i % 13], dtype=np.float32).tobytes(), (n, i)
    script = tmp_path / "wpc.py"
    script.write_text(f"""
import sys, hashlib
import numpy as np
sys.path.insert(0, {ROOT!r})
import prosody_control_french_tts_amd as P
from prosody_control_french_tts_amd import synth, whisper_weights as WW
from prosody_control_french_tts_amd.Aligners import decoding as DEC
from tests.test_whisper_hf_crosscheck import _greedy_gold
_, rules = _greedy_gold()
init = _greedy_gold()[0]["initial"].tolist()
edims = dict(n_mels=80, n_ctx=1500, n_state={D}, n_head={H}, n_layer=1)
tdims = dict(n_vocab=300, n_text_ctx=96, n_state={D}, n_head={H}, n_layer=2)
We, Wd = WW.synthetic_weights(edims, seed=31), WW.greedy_test_decoder_weights(tdims, seed=33)
use = [synth.synth_clip(60 + i, seconds=1.5 + 0.5 * (i % 3)) for i in range(5)]
with P.ProsodyEngine(0) as eng:
    eng.upload(use, 16000); eng.logmel_run(80)
    eng.whisper_load(edims, WW.pack(We, edims)); eng.whisper_encode_run()
    eng.whisper_decoder_load(tdims, WW.pack_decoder(Wd, tdims))
    t, l = DEC.decode_batch(eng, 300, [list(init)] * 5, [len(init)] * 5, rules, sample_len=6)[:2]
h = hashlib.sha1()
for a, b in zip(t, l):
    h.update(np.asarray(a, dtype=np.int64).tobytes()); h.update(np.asarray(b, dtype=np.float32).tobytes())
print("HASH", h.hexdigest(), [len(a) for a in t])
""")
    seen = {}
    for wpc in (4, 2, 1):
        r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, PCE_XATTN_WPC=str(wpc)), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        seen[wpc] = [ln for ln in r.stdout.splitlines() if ln.startswith("HASH")][0]
    assert len(set(seen.values())) == 1, seen


def test_row_major_self_attention_caches_at_20_heads():
    """``k_self_attn1w`` in two head groups of 10 waves (row-major K / V caches, each group appending its own heads' columns) against
    ``PCE_SELF_ROWS=0`` (``k_cross_attn1w`` on K rows + V^T, also in head groups): the same tokens, log-probabilities within 0.02."""
    init, _ = _gold()
    n = 4
    edims = dict(n_mels=80, n_ctx=1500, n_state=D, n_head=H, n_layer=1)
    tdims = dict(n_vocab=300, n_text_ctx=96, n_state=D, n_head=H, n_layer=3)
    We, Wd = WW.synthetic_weights(edims, seed=377), WW.greedy_test_decoder_weights(tdims, seed=379)
    use = [synth.synth_clip(120 + i, seconds=2.0 + i) for i in range(n)]
    prompts = [[7, 13][: i % 2 + 1] * (i + 1) + list(init) for i in range(n)]
    runs = {}
    for form in ("1", "0"):
        eng = _fresh_engine(PCE_SELF_ROWS=form)
        try:
            runs[form] = _decode(eng, edims, tdims, We, Wd, use, prompts, [len(p) for p in prompts], 10)[:2]
        finally:
            eng.close()
    (ta, la), (tb, lb) = runs["1"], runs["0"]
    for i in range(n):
        assert ta[i] == tb[i], (i, ta[i], tb[i])
        assert len(ta[i]) >= 3 and np.allclose(la[i], lb[i], atol=0.02), (i, la[i], lb[i])


def test_one_context_decodes_1024_then_1280_then_768(engine):
    """Each width's ``k_xattn_absorbed`` instantiation carries its own dynamic-LDS attribute (136 KB at d = 1280): one context decodes the three
    widths in turn."""
    init, rules = _gold()
    from prosody_control_french_tts_amd.Aligners import decoding as DEC
    use = [synth.synth_clip(60 + i, seconds=2.0) for i in range(2)]
    for d, heads in ((1024, 16), (1280, 20), (768, 12)):
        edims = dict(n_mels=80, n_ctx=1500, n_state=d, n_head=heads, n_layer=1)
        tdims = dict(n_vocab=300, n_text_ctx=96, n_state=d, n_head=heads, n_layer=1)
        engine.upload(use, 16000); engine.logmel_run(80)
        engine.whisper_load(edims, WW.pack(WW.synthetic_weights(edims, seed=5), edims)); engine.whisper_encode_run()
        engine.whisper_decoder_load(tdims, WW.pack_decoder(WW.greedy_test_decoder_weights(tdims, seed=6), tdims))
        toks, lps, _ = DEC.decode_batch(engine, tdims["n_vocab"], [list(init)] * 2, [len(init)] * 2, rules, sample_len=5)
        assert all(1 <= len(t) <= 5 for t in toks) and all(np.isfinite(l).all() for l in lps), d


def test_logmel_and_encoder_with_128_mels(engine, ops):
    """The large-v3 front end: 128 mel bands against ``WO.log_mel(c, 128)`` (2e-3, as at 80), and a 2-layer d = 1280 encoder fed by them against the
    torch restatement with the bounds of tests/test_gpu_whisper.py's encoder test."""
    rng = np.random.default_rng(5)
    clips = [synth.synth_clip(0, seconds=10.0), (rng.standard_normal(16000 * 31) * 2500).astype(np.int16)]
    dims = dict(WW.DIMS["turbo"], n_layer=2)
    engine.upload(clips, 16000)
    engine.logmel_run(128)
    for i, c in enumerate(clips):
        got = engine.logmel_fetch(i)
        want = WO.log_mel(c[:WO.N_SAMPLES], 128)
        assert got.shape == want.shape == (128, 3000)
        assert np.max(np.abs(got - want)) <= 2e-3, (i, np.max(np.abs(got - want)))
    W = WW.synthetic_weights(dims)
    engine.whisper_load(dims, WW.pack(W, dims))
    engine.whisper_encode_run()
    for i in range(2):
        got = engine.whisper_encode_fetch(i)
        want = WO.encoder_forward(WO.log_mel(clips[i], 128), W, dims)
        assert got.shape == want.shape == (1500, 1280)
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert rel <= ops["enc_l2"], (ops["name"], rel)
        worst = np.max(np.abs(got - want)) / max(1.0, float(np.std(want)))
        assert worst <= ops["enc_max"], (ops["name"], worst)


def test_aligner_end_to_end_with_a_turbo_checkpoint(engine, tmp_path, monkeypatch):
    """``use_whisper_timestamped.main(..., whisper_model="turbo")`` -- the reference aligner's default model name -- from a directory holding
    turbo.npz (d = 1280, 20 heads, 128 mels, 4 decoder layers, one more language token) and multilingual.tiktoken: the built-in turbo alignment
    heads (layers 2-3) drive the DTW, and the file contract is the one tests/test_gpu_aligner.py checks, a 33 s recording included."""
    import base64
    from prosody_control_french_tts_amd import engine as E
    from prosody_control_french_tts_amd.Aligners import checkpoint as CK
    from prosody_control_french_tts_amd.Aligners import use_whisper_timestamped as A
    from tests.test_gpu_aligner import _assert_aligner_outputs, toy_tokenizer, write_wav
    root = tmp_path / "whisper_dir"
    root.mkdir()
    tk = toy_tokenizer()
    edims = dict(WW.DIMS["turbo"], n_layer=2)
    tdims = dict(WW.TEXT_DIMS["turbo"], n_vocab=tk.n_vocab + 1, n_text_ctx=128)
    enc, dec = WW.synthetic_weights(edims, seed=77), WW.greedy_test_decoder_weights(tdims, seed=79)
    np.savez(root / "turbo.npz", **{"encoder." + k: v for k, v in enc.items()}, **{"decoder." + k: v for k, v in dec.items()})
    with open(root / "multilingual.tiktoken", "wb") as f:
        for tok, rank in tk.ranks.items():
            f.write(base64.b64encode(tok) + b" " + str(rank).encode() + b"\n")
    m = CK.load_model("turbo", str(root))
    assert sorted(map(tuple, np.argwhere(m.alignment_heads).tolist())) == [(2, 4), (2, 11), (3, 3), (3, 6), (3, 11), (3, 14)]
    monkeypatch.setenv("PCE_WHISPER_DIR", str(root))
    A.set_model_source()
    E.set_default_engine(engine)
    voice = tmp_path / "Data" / "V9"
    audio = voice / "audio"; audio.mkdir(parents=True)
    write_wav(audio / "segment_ph1.wav", synth.synth_clip(3, seconds=5.0))
    write_wav(audio / "segment_ph2.wav", np.zeros(20000, np.int16))                                  # gated: silence
    write_wav(audio / "segment_ph4.wav", np.concatenate([synth.synth_clip(20 + k, seconds=3.0) for k in range(11)]))   # 33 s: two windows
    out = voice / "WhisperTS_textgrid_files"
    try:
        A.main(str(audio), str(out), whisper_model="turbo", device="cuda:0", logger=logging.getLogger("t"))
    finally:
        E.set_default_engine(None)
        A.set_model_source()
    names = ["segment_ph1", "segment_ph2", "segment_ph4"]
    for n in names:
        assert (out / f"{n}.TextGrid").exists() and (Path(str(out) + "_transcription") / f"{n}.txt").exists()
    _assert_aligner_outputs(audio, out, names, gated=("segment_ph2",))
    raw4 = json.loads((Path(str(out) + "_raw_json") / "segment_ph4.raw.json").read_text(encoding="utf-8"))
    if raw4["text"] != "...":
        assert max(s["end"] for s in raw4["segments"]) > 30.0
