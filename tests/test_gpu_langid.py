"""Whisper language detection on the device (``pce_whisper_detect_language`` / ``k_lang_probs``) and ``language=None`` end to end.

Pinned to the ``transformers`` forward by tests/golden/whisper_langid_tiny.npz (made by tests/golden/make_goldens_langid.py: the mask / softmax
rule on top of it is a restatement of openai-whisper's ``detect_language``); checked against the engine's own full output projection (the
no-speech probe of ``whisper_decode_step_ex``), for batch independence bit by bit, at the shapes where the kernel takes another turn, for ties,
for its error returns, for leaving the decoding calls that follow untouched, and through ``transcribe_batch(language=None)``."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_goldens_langid as G  # noqa: E402
from oracle import whisper_oracle as WO  # noqa: E402
from prosody_control_french_tts_amd import synth, whisper_weights as WW  # noqa: E402
from prosody_control_french_tts_amd.Aligners import checkpoint as CK, decoding as DEC, transcribe as TR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "whisper_langid_tiny.npz"))


@pytest.fixture(scope="module")
def clips(gold):
    every = G.clips()
    return [every[int(i)] for i in gold["clips"]]


_WEIGHTS = {}


def weights(gold, num_languages):
    """(tokenizer, text dims, encoder weights, decoder weights) of the golden's miniature for one vocabulary: made once, never changed."""
    if num_languages not in _WEIGHTS:
        tk = G.tokenizer(num_languages)
        tdims = G.text_dims(tk)
        assert tk.n_vocab == int(gold[f"n_vocab_{num_languages}"][0]) and tk.sot == int(gold[f"sot_{num_languages}"][0])
        _WEIGHTS[num_languages] = (tk, tdims, WW.synthetic_weights(G.EDIMS, seed=int(gold["encoder_seed"][0])),
                                   G.decoder_weights(tk, tdims, int(gold[f"seed_{num_languages}"][0])))
    return _WEIGHTS[num_languages]


def encode(engine, clips, edims, We, tdims, Wd):
    engine.upload(list(clips), 16000)
    engine.logmel_run(edims["n_mels"])
    engine.whisper_load(edims, WW.pack(We, edims))
    engine.whisper_encode_run()
    engine.whisper_decoder_load(tdims, WW.pack_decoder(Wd, tdims))


def detect(engine, tk):
    lang = tk.all_language_tokens
    return engine.whisper_detect_language(tk.sot, lang[0], len(lang))


# ------------------------------------------------------------------------------------------------------------------ 1. golden
@pytest.mark.parametrize("num_languages", [99, 100])
def test_golden_transformers_logits(engine, ops, gold, clips, num_languages):
    """ids equal for EVERY clip, probabilities within the bound tests/test_gpu_aligner.py applies to the no-speech probe (the same decoder
    pass, the same operand rounding): |got - want| <= 0.02 max(want, 1e-3) + 1e-5 (make_goldens_langid.tolerance; the golden's top-2 margins
    are ten times that)."""
    tk, tdims, We, Wd = weights(gold, num_languages)
    encode(engine, clips, G.EDIMS, We, tdims, Wd)
    ids, probs = detect(engine, tk)
    want = gold[f"probs_{num_languages}"]
    assert probs.shape == want.shape == (len(clips), num_languages) and probs.dtype == np.float32 and ids.dtype == np.int32
    err = np.abs(probs.astype(np.float64) - want)
    print(f"langid golden {ops['name']} n_lang={num_languages}: worst |dp| / bound = {np.max(err / G.tolerance(want)):.4f}, worst |dp| = {err.max():.3e}")
    assert np.array_equal(ids, gold[f"ids_{num_languages}"]), (ids, gold[f"ids_{num_languages}"])
    assert np.all(gold[f"margin_{num_languages}"] >= 10.0 * G.tolerance(want.max(-1)))
    assert np.all(err <= G.tolerance(want)), float(np.max(err / G.tolerance(want)))
    assert np.all(np.abs(probs.sum(-1, dtype=np.float64) - 1.0) <= 1e-5)
    assert len(set(ids.tolist())) >= 2


# ------------------------------------------------------------------------------------------- 2. (and 4.) the engine's own projection
def _round_operands(x, name):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.bfloat16 if name == "bf16" else torch.float16).double().numpy()


def _against_full_projection(engine, ops_name, tk, tdims, Wd, n):
    """-> (probabilities of the new kernel, of the full projection, the float64 reference), each [clips][n_lang].  Reference: softmax over the
    language tokens of the float64 dot products of the operands as the device holds them -- the hidden state of the <|startoftranscript|>
    position (the float32 restatement's, on the device's own encoder output) and the embedding rows, both rounded to the operand type."""
    lang = np.asarray(tk.all_language_tokens)
    ids, probs = detect(engine, tk)
    rules = tk.decoding_rules()
    mask = DEC.vocab_mask(tdims["n_vocab"], rules["suppress_tokens"], rules["blank_tokens"], rules["no_timestamps"])
    probe = np.zeros((n, len(lang)), dtype=np.float64)
    for k, t in enumerate(lang):
        _, _, pr = engine.whisper_decode_step_ex([[tk.sot]] * n, 1, rules["eot"], rules["timestamp_begin"], mask, probe_token=int(t))
        probe[:, k] = pr
    full = probe / probe.sum(-1, keepdims=True)
    emb = _round_operands(Wd["token_embedding.weight"][lang], ops_name)
    ref = np.zeros_like(full)
    for i in range(n):
        hidden = WO.find_alignment([tk.sot], engine.whisper_encode_fetch(i), Wd, tdims, 2, 0, want_internal=True)["hidden"][-1]
        logit = emb @ _round_operands(hidden, ops_name)
        e = np.exp(logit - logit.max())
        ref[i] = e / e.sum()
    assert np.array_equal(ids, lang[np.argmax(probs, -1)])
    return probs.astype(np.float64), full, ref


def _check_against_full_projection(label, new, full, ref, few):
    d_new, d_full = float(np.abs(new - ref).max()), float(np.abs(full - ref).max())
    print(f"langid vs full projection {label}: distance to float64  new kernel {d_new:.3e}  full projection {d_full:.3e}  |new - full| {np.abs(new - full).max():.3e}")
    # the new kernel at most as far from float64 as the existing logits path on the same inputs, times two for the accumulation order
    assert d_new <= 2.0 * d_full, (d_new, d_full)
    for t in few:                                                      # probs[t] = probe(t) / sum over the languages of probe, within those two distances
        assert np.all(np.abs(new[:, t] - full[:, t]) <= d_new + d_full), t


@pytest.mark.parametrize("num_languages", [99, 100])
def test_equals_the_full_projection(engine, ops, gold, clips, num_languages):
    """n_lang = 99 and 100 (neither a multiple of the 64 lanes nor of the 8 waves) at the miniature width (128: lanes 16..63 sit every round out)."""
    tk, tdims, We, Wd = weights(gold, num_languages)
    encode(engine, clips, G.EDIMS, We, tdims, Wd)
    new, full, ref = _against_full_projection(engine, ops["name"], tk, tdims, Wd, len(clips))
    _check_against_full_projection(f"{ops['name']} d=128 n_lang={num_languages}", new, full, ref, few=(0, 6, 63, 64, num_languages - 1))


def test_width_1280_twenty_heads(engine, ops):
    """large-v3 / turbo width: d = 1280 (two and a half rounds of 512 columns per row), one layer, 20 heads, two clips, 100 languages."""
    tk = G.tokenizer(100)
    edims = dict(n_mels=80, n_ctx=1500, n_state=1280, n_head=20, n_layer=1)
    tdims = dict(n_vocab=tk.n_vocab, n_text_ctx=32, n_state=1280, n_head=20, n_layer=1)
    We, Wd = WW.synthetic_weights(edims, seed=77), G.decoder_weights(tk, tdims, 81)
    two = [synth.synth_clip(5, seconds=2.0), np.zeros(16000, dtype=np.int16)]
    encode(engine, two, edims, We, tdims, Wd)
    new, full, ref = _against_full_projection(engine, ops["name"], tk, tdims, Wd, 2)
    _check_against_full_projection(f"{ops['name']} d=1280 n_lang=100", new, full, ref, few=(0, 6, 63, 64, 99))


def test_one_language_is_certain(engine, gold, clips):
    tk, tdims, We, Wd = weights(gold, 99)
    encode(engine, clips, G.EDIMS, We, tdims, Wd)
    for t in (tk.all_language_tokens[0], tk.all_language_tokens[70], tdims["n_vocab"] - 1):
        ids, probs = engine.whisper_detect_language(tk.sot, int(t), 1)
        assert np.array_equal(ids, np.full(len(clips), t, dtype=np.int32)) and np.array_equal(probs, np.ones((len(clips), 1), dtype=np.float32))
    ids, probs = engine.whisper_detect_language(tk.sot, tk.all_language_tokens[0], 64)          # (exactly the lanes of one wave)
    ids99, probs99 = detect(engine, tk)
    assert np.all(np.abs(probs.sum(-1, dtype=np.float64) - 1.0) <= 1e-5)
    lo = probs99[:, :64].astype(np.float64)
    assert np.all(np.abs(probs - lo / lo.sum(-1, keepdims=True)) <= 1e-6)


# --------------------------------------------------------------------------------------------------------- 3. batch independence
def test_batch_independence_bitwise(engine, ops, gold, clips):
    tk, tdims, We, Wd = weights(gold, 100)
    subject = clips[4]
    filler = [synth.synth_clip(10 + k, seconds=2.0) for k in range(16)]
    encode(engine, [subject], G.EDIMS, We, tdims, Wd)
    ids0, probs0 = detect(engine, tk)
    for n in (3, 17):
        for at in (0, n - 1):
            batch = filler[:n - 1]
            batch.insert(at, subject)
            encode(engine, batch, G.EDIMS, We, tdims, Wd)
            ids, probs = detect(engine, tk)
            assert ids[at] == ids0[0] and probs[at].tobytes() == probs0[0].tobytes(), (n, at)


# ------------------------------------------------------------------------------------------------------------------ 5. ties
def test_ties_go_to_the_lower_id(engine, ops, gold, clips):
    tk, tdims, We, Wd = weights(gold, 99)
    lang = np.asarray(tk.all_language_tokens)
    winners = sorted(set(int(t) for t in gold["ids_99"]))
    twin = {}                                                          # every winning row gets an identical twin at a lower language id
    emb = Wd["token_embedding.weight"].copy()
    free = [int(t) for t in lang if int(t) not in winners]
    for k, w in enumerate(winners):
        lower = [t for t in free if t < w]
        twin[w] = lower[k]
        emb[twin[w]] = emb[w]
    assert len(set(twin.values())) == len(winners)
    encode(engine, clips, G.EDIMS, We, tdims, dict(Wd, **{"token_embedding.weight": emb}))
    ids, probs = detect(engine, tk)
    for i, w in enumerate(int(t) for t in gold["ids_99"]):
        assert int(ids[i]) == twin[w], (i, int(ids[i]), w, twin[w])
        assert probs[i, twin[w] - lang[0]].tobytes() == probs[i, w - lang[0]].tobytes()
        assert probs[i, w - lang[0]] == probs[i].max()


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def test_error_returns(gold, clips):
    import prosody_control_french_tts_amd as P
    tk, tdims, We, Wd = weights(gold, 99)
    lang = tk.all_language_tokens
    eng = P.ProsodyEngine(0)
    try:
        with pytest.raises(P.PceError, match="status -4"):                                         # PCE_E_STATE: no decoder yet
            eng.whisper_detect_language(tk.sot, lang[0], len(lang))
        eng.whisper_load(G.EDIMS, WW.pack(We, G.EDIMS))
        eng.whisper_decoder_load(tdims, WW.pack_decoder(Wd, tdims))
        with pytest.raises(P.PceError, match="status -4"):                                         # PCE_E_STATE: nothing encoded
            eng.whisper_detect_language(tk.sot, lang[0], len(lang))
        eng.upload(clips[3:], 16000); eng.logmel_run(80); eng.whisper_encode_run()
        for begin, count in ((lang[0], 0), (lang[0], 129), (lang[0], -1), (tdims["n_vocab"] - 98, 99), (-1, 99)):
            with pytest.raises(P.PceError, match="status -1"):                                     # PCE_E_INVALID
                eng.whisper_detect_language(tk.sot, begin, count)
        with pytest.raises(P.PceError, match="status -1"):
            eng.whisper_detect_language(tdims["n_vocab"], lang[0], len(lang))
        ids, probs = detect(eng, tk)                                                               # the context is usable afterwards
        assert np.array_equal(ids, gold["ids_99"][3:]) and np.all(np.abs(probs - gold["probs_99"][3:]) <= G.tolerance(gold["probs_99"][3:]))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 7. no side effect on decoding
def test_decoding_after_detection_is_unchanged(engine, ops, gold, clips):
    tk, tdims, We, Wd = weights(gold, 100)
    rules = tk.decoding_rules()
    mask = DEC.vocab_mask(tdims["n_vocab"], rules["suppress_tokens"], rules["blank_tokens"], rules["no_timestamps"])
    prompts = [list(tk.sot_sequence("fr")), [tk.sot_prev, 66, 67] + list(tk.sot_sequence("de")), list(tk.sot_sequence("en"))]
    begins = [len(p) for p in prompts]
    use = [clips[4], clips[1], clips[0]]

    def loop():
        return engine.whisper_decode_loop(prompts, begins, rules["eot"], rules["timestamp_begin"], mask, 12, rules["max_initial_timestamp_index"],
                                          probe_token=tk.no_speech)
    encode(engine, use, G.EDIMS, We, tdims, Wd)
    t0, lp0, pr0 = loop()
    encode(engine, use, G.EDIMS, We, tdims, Wd)
    detect(engine, tk)
    t1, lp1, pr1 = loop()
    assert t0.shape[1] >= 2 and np.array_equal(t0, t1) and lp0.tobytes() == lp1.tobytes() and pr0.tobytes() == pr1.tobytes()
    detect(engine, tk)                                                                             # ... and between two host-driven steps
    s1 = engine.whisper_decode_step_ex(prompts, begins, rules["eot"], rules["timestamp_begin"], mask, rules["max_initial_timestamp_index"])
    assert np.array_equal(s1[0], t0[:, 0]) and s1[1].tobytes() == lp0[:, 0].tobytes()


# ------------------------------------------------------------------------------------------------------------ 8. end to end
def test_transcribe_without_a_language(engine, gold, clips):
    tk, tdims, We, Wd = weights(gold, 100)
    model = CK.WhisperModel(dict(We), dict(Wd), alignment_heads=[[1, 0], [1, 1]], name="toy").load_into(engine)
    codes = [tk.all_language_codes[int(t) - tk.all_language_tokens[0]] for t in gold["ids_100"]]
    assert len(set(codes)) >= 2

    def run(language):
        opts = TR.TranscribeOptions(language=language, vad=None, detect_disfluencies=False, sample_len=10, max_windows=2, logprob_threshold=None,
                                    no_speech_threshold=None, compression_ratio_threshold=None)
        return TR.transcribe_batch(engine, model, tk, clips, opts)
    auto = run(None)
    assert [r["language"] for r in auto] == codes
    strip = lambda r: [(s["seek"], s["tokens"], s["avg_logprob"], s["start"], s["end"], [(w["text"], w["start"], w["end"]) for w in s["words"]]) for s in r["segments"]]
    assert any(r["segments"] for r in auto)
    for code in sorted(set(codes)):
        given = run(code)
        assert all(r["language"] == code for r in given)
        for i, c in enumerate(codes):
            if c == code:
                assert strip(auto[i]) == strip(given[i]), (i, code)
