"""GPU tests of pce_ctc_align (csrc/pce_ctc.hip) through ``ProsodyEngine.ctc_align`` and ``Aligners/CTCFA.process_files``.  Every
comparison is exact: path, tok_first, tok_last and status equal those of the CPU restatement (tests/ctc_restatement.py), frame_score
and score equal its float32 bits.  Inputs are seeded log-softmax rows; a second set is quantised to multiples of 0.25 (ties everywhere)."""
import os
import wave

import numpy as np
import pytest
import torch  # noqa: F401  (before the session's engine loads libpce.so: torch brings its own copy of the HIP runtime, and the one loaded first serves both)

import ctc_restatement as CR

pytestmark = pytest.mark.gpu

RUN, WAVE_STATES, TWO_WAVES, LIMIT = 4, 256, 512, 4096        # states per thread, per wave, per two waves; the register form's limit
FRAMES = (1, 2, 3, 63, 64, 65, 257)


def emissions(rng, T, V, quantised, star):
    """[T, V] log-softmax rows; star: the last column is the zero column of the <star> token (outside the softmax)."""
    n = V - 1 if star else V
    x = rng.standard_normal((T, n)) * (0.7 if quantised else 2.0)
    lp = (x - np.log(np.sum(np.exp(x), axis=1, keepdims=True))).astype(np.float32)
    if quantised:
        lp = (np.round(lp * 4) / 4).astype(np.float32)
    return np.concatenate([lp, np.zeros((T, 1), np.float32)], axis=1) if star else lp


def targets_with(rng, L, V, repeats):
    """L labels in [1, V), no two neighbours equal except `repeats` pairs at the front."""
    t = np.zeros(L, dtype=np.int32)
    for l in range(L):
        t[l] = rng.integers(1, V)
        while l and t[l] == t[l - 1]:
            t[l] = rng.integers(1, V)
    for r in range(min(repeats, L - 1)):
        t[2 * r + 1] = t[2 * r]
        if 2 * r + 2 < L and t[2 * r + 2] == t[2 * r + 1]:
            t[2 * r + 2] = t[2 * r + 1] % (V - 1) + 1
    return t


def boundary_cases():
    """2 L + 1 one below / at / one above each boundary of the register form (2 L + 1 is odd: the odd ones of the three), every T of FRAMES
    plus the clip's shortest T and a few frames more, V = 8 and V = 41 (with the star column), plain and quantised rows."""
    rng = np.random.default_rng(18)
    cases = []
    for states in (RUN - 1, RUN + 1, WAVE_STATES - 1, WAVE_STATES + 1, TWO_WAVES - 1, TWO_WAVES + 1, LIMIT - 1):
        L = (states - 1) // 2
        for V in (8, 41):
            for quantised in (False, True):
                tg = targets_with(rng, L, V, repeats=1)
                need = L + CR.n_repeats(tg)
                frames = sorted(set(FRAMES) | {need, need + 5}) if states < LIMIT - 1 else [need + 5]
                for T in frames:
                    cases.append((emissions(rng, T, V, quantised, star=V == 41), tg))
    return cases


@pytest.fixture(scope="module")
def boundary():
    cases = boundary_cases()
    return cases, [CR.forced_align(lp, tg) for lp, tg in cases]


def mixed_cases():
    """33 clips, T in 1 .. 300, V = 8.  Odd clips: any T, L up to T / 2 with the repeats chance brings.  Even clips: T near 300 with L just
    below it (up to 599 states: two and three waves), so that the batch's trace passes 1 MiB (test 6)."""
    rng = np.random.default_rng(33)
    cases = []
    for k in range(33):
        if k % 2 == 0:
            tg = targets_with(rng, 300 - 5 * (k // 2) - 3, 8, repeats=k % 3)
            T = len(tg) + CR.n_repeats(tg) + int(rng.integers(0, 3))
        else:
            T = int(rng.integers(1, 301))
            tg = rng.integers(1, 8, size=int(rng.integers(1, max(2, T // 2)))).astype(np.int32)
        assert 1 <= T <= 300
        cases.append((emissions(rng, T, 8, quantised=bool(k & 2), star=False), tg))
    return cases


@pytest.fixture(scope="module")
def mixed():
    cases = mixed_cases()
    return cases, [CR.forced_align(lp, tg) for lp, tg in cases]


def check(got, want, what=""):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert CR.same_result(g, w), (what, k, len(w["path"]), len(w["tok_first"]), g["status"], w["status"], g["score"], w["score"])


# ------------------------------------------------------------------ 1 + 2. shapes around every boundary, both forms
def test_boundary_shapes_register_form(engine, boundary):
    cases, want = boundary
    assert {w["status"] for w in want} == {CR.OK, CR.TOO_SHORT}
    engine.profile_enable(True); engine.profile_reset()
    got = engine.ctc_align([c[0] for c in cases if c[0].shape[1] == 8], [c[1] for c in cases if c[0].shape[1] == 8], form="register")
    prof = engine.profile(); engine.profile_enable(False)
    assert "k_ctc" in prof and "k_ctc_trace" in prof and "k_ctc_general" not in prof
    check(got, [w for c, w in zip(cases, want) if c[0].shape[1] == 8], "V = 8")
    sel = [k for k, c in enumerate(cases) if c[0].shape[1] == 41]
    check(engine.ctc_align([cases[k][0] for k in sel], [cases[k][1] for k in sel]), [want[k] for k in sel], "V = 41")
    assert any(40 in cases[k][1] for k in sel)                     # the star column is a target somewhere


def test_boundary_shapes_general_form(engine, boundary):
    cases, want = boundary
    for V in (8, 41):
        sel = [k for k, c in enumerate(cases) if c[0].shape[1] == V]
        engine.profile_enable(True); engine.profile_reset()
        got = engine.ctc_align([cases[k][0] for k in sel], [cases[k][1] for k in sel], form="general")
        prof = engine.profile(); engine.profile_enable(False)
        assert "k_ctc_general" in prof and "k_ctc" not in prof
        check(got, [want[k] for k in sel], f"general, V = {V}")


def test_over_the_limit_takes_the_general_form(engine):
    import prosody_control_french_tts_amd as P
    rng = np.random.default_rng(4097)
    tg = targets_with(rng, LIMIT // 2, 8, repeats=1)              # 4097 states
    lp = emissions(rng, len(tg) + 1 + 4, 8, quantised=True, star=False)
    small = (emissions(rng, 9, 8, False, False), np.array([1, 2, 2], np.int32))
    engine.profile_enable(True); engine.profile_reset()
    got = engine.ctc_align([small[0], lp, small[0]], [small[1], tg, small[1]])
    prof = engine.profile(); engine.profile_enable(False)
    assert prof["k_ctc_general"]["launches"] == 1 and prof["k_ctc"]["launches"] == 1
    check(got, [CR.forced_align(*small), CR.forced_align(lp, tg), CR.forced_align(*small)])
    with pytest.raises(P.PceError, match="status -5"):
        engine.ctc_align([small[0], lp], [small[1], tg], form="register")


# ------------------------------------------------------------------ 3. statuses
def test_statuses_and_their_neighbours(engine):
    import prosody_control_french_tts_amd as P
    rng = np.random.default_rng(3)
    V = 8
    ok = lambda: (emissions(rng, 40, V, False, False), rng.integers(1, V, size=9).astype(np.int32))
    rep = np.array([3, 3, 3], np.int32)                            # L + R = 5
    blocked = emissions(rng, 6, V, False, False)
    blocked[2, :] = -np.inf                                         # every route crosses frame 2
    half = emissions(rng, 6, V, False, False)
    half[:, 5] = -np.inf                                            # the only label the clip needs at some frame
    clips = [ok(), (emissions(rng, 12, V, False, False), np.zeros(0, np.int32)), ok(), (np.zeros((0, V), np.float32), np.array([1, 2], np.int32)), ok(),
             (emissions(rng, 4, V, True, False), rep), ok(), (emissions(rng, 5, V, True, False), rep), ok(), (blocked, np.array([1, 2], np.int32)), ok(),
             (half, np.array([5], np.int32)), ok(), (emissions(rng, 7, V, True, False), rep)]
    want = [CR.forced_align(lp, tg) for lp, tg in clips]
    assert [w["status"] for w in want] == [0, CR.EMPTY, 0, CR.EMPTY, 0, CR.TOO_SHORT, 0, CR.OK, 0, CR.NO_PATH, 0, CR.NO_PATH, 0, CR.OK]
    assert want[7]["path"].tolist() == [3, 0, 3, 0, 3] and want[9]["score"] == -np.inf
    for form in ("auto", "general"):
        check(engine.ctc_align([c[0] for c in clips], [c[1] for c in clips], form=form), want, form)
    alone = engine.ctc_align([clips[0][0]], [clips[0][1]])
    check(alone, want[:1])
    for bad in ([1, 0, 2], [1, V], [-1]):                           # the blank, past the vocabulary, negative
        with pytest.raises(P.PceError, match="status -1"):
            engine.ctc_align([clips[0][0], clips[2][0]], [clips[0][1], np.array(bad, np.int32)])
    got = engine.ctc_align([clips[7][0]], [rep], return_path=False)
    assert "path" not in got[0] and got[0]["tok_first"].tolist() == [0, 2, 4] and got[0]["score"] == want[7]["score"]


# ------------------------------------------------------------------ 4. batch independence
def test_batch_independence(engine, mixed):
    cases, want = mixed
    together = engine.ctc_align([c[0] for c in cases], [c[1] for c in cases])
    check(together, want, "together")
    backwards = engine.ctc_align([c[0] for c in cases[::-1]], [c[1] for c in cases[::-1]])
    check(backwards[::-1], want, "reverse order")
    for k, c in enumerate(cases):
        check(engine.ctc_align([c[0]], [c[1]]), [want[k]], f"alone {k}")
    assert sum(w["status"] == CR.OK for w in want) >= 25


# ------------------------------------------------------------------ 5. input forms
def test_input_forms(engine, mixed):
    cases, want = mixed
    cases, want = cases[:12], want[:12]
    t_max, V = max(c[0].shape[0] for c in cases), 8
    padded = np.full((len(cases), t_max, V), -1.0, np.float32)     # the padding rows hold a value no clip may read
    for k, c in enumerate(cases):
        padded[k, :len(c[0])] = c[0]
    n_frames = np.array([len(c[0]) for c in cases], np.int32)
    tg = [c[1] for c in cases]
    check(engine.ctc_align(torch.from_numpy(padded), tg, n_frames=n_frames), want, "CPU tensor")
    dev = torch.from_numpy(padded).to("cuda:0")
    keep = dev.clone()
    check(engine.ctc_align(dev, tg, n_frames=torch.from_numpy(n_frames)), want, "ROCm tensor")
    assert torch.equal(dev, keep)
    check(engine.ctc_align([c[0] for c in cases], tg), want, "list")
    with pytest.raises(ValueError):
        engine.ctc_align(dev[:, :, :4], tg, n_frames=n_frames)    # not contiguous
    with pytest.raises(ValueError):
        engine.ctc_align(dev.double(), tg, n_frames=n_frames)


# ------------------------------------------------------------------ 6. trace budget
def test_trace_budget_splits_the_batch(monkeypatch, mixed):
    import prosody_control_french_tts_amd as P
    cases, want = mixed
    monkeypatch.setenv("PCE_CTC_TRACE_MB", "1")
    with P.ProsodyEngine(0) as small:
        small.profile_enable(True); small.profile_reset()
        got = small.ctc_align([c[0] for c in cases], [c[1] for c in cases])
        groups = small.profile()["k_ctc_trace"]["launches"]
        check(got, want, "1 MiB of trace")
        # ceil(T / 4) words per sweeping thread: the 17 long clips hold 256 threads x 55 .. 75 words x 4 bytes each, 1.1 MiB together
        assert groups >= 2
        rng = np.random.default_rng(1)
        tg = targets_with(rng, 2047, 8, repeats=0)                  # 1 024 threads x ceil(2060 / 4) words = 2.0 MiB
        with pytest.raises(P.PceError, match="status -5"):
            small.ctc_align([np.zeros((2060, 8), np.float32), cases[1][0]], [tg, cases[1][1]])


# ------------------------------------------------------------------ 7. end to end
def test_process_files_end_to_end(engine, tmp_path, capsys):
    import transformers
    from prosody_control_french_tts_amd import synth
    from prosody_control_french_tts_amd.Aligners import CTCFA, ctc_emissions, ctc_segments
    from prosody_control_french_tts_amd.textgrid_io import read_textgrid
    torch.manual_seed(0)
    cfg = transformers.Wav2Vec2Config(vocab_size=32, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                      conv_dim=(16,) * 7, num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=2)
    model = transformers.Wav2Vec2ForCTC(cfg).eval().to("cuda:0")
    vocab = {ch: i + 1 for i, ch in enumerate("abcdefghijklmnopqrstuvwxyz'")}
    texts = {"c0": "Bonjour, le monde!", "c1": "la (petite) maison: bleue", "c2": "il arrive — demain"}
    audio, trans, out = tmp_path / "audio", tmp_path / "txt", tmp_path / "tg"
    audio.mkdir(); trans.mkdir()
    clips = {}
    for k, name in enumerate(sorted(texts)):
        clips[name] = synth.synth_clip(k, seconds=2.0 + 0.5 * k)
        with wave.open(str(audio / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(clips[name].tobytes())
        (trans / f"{name}.txt").write_text(texts[name], encoding="utf-8")
    with wave.open(str(audio / "orphan.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(clips["c0"].tobytes())
    rows = CTCFA.process_files(str(audio), str(trans), str(out), "fra", "segment", False, engine=engine, model=model, vocab=vocab)
    said = capsys.readouterr().out
    assert f"Missing transcription file: {trans / 'orphan.txt'}" in said and said.count("Processed file : ") == 3
    names = sorted(texts)
    em, n_frames = ctc_emissions.hf_emissions(model, [clips[n] for n in names], torch.device("cuda", 0))
    assert em.shape[2] == 33 and n_frames.tolist() == [100, 125, 150]
    def grid_words(directory, name):
        tg = read_textgrid(os.path.join(directory, f"{name}.TextGrid"))
        assert [t.name for t in tg.tiers] == ["Mots"]
        return [iv for iv in tg.tiers[0].intervals if iv[2] != ""]
    for name in names:
        words = ctc_segments.preprocess_text(texts[name].lower()).split()
        got = grid_words(str(out), name)
        assert [iv[2] for iv in got] == words == [r["text"] for r in rows[f"{name}.wav"]]
        duration = len(clips[name]) / 16000
        assert all(0 <= a < b <= duration for a, b, _ in got) and all(x[1] <= y[0] for x, y in zip(got, got[1:]))
        assert os.path.exists(audio / f"{name}.txt") and not os.path.exists(trans / f"{name}_clean.txt")
    # the same files from the emissions above, against ctc_segments on the restatement's path over those emissions fetched to the host
    out2 = tmp_path / "tg2"
    CTCFA.process_files(str(audio), str(trans), str(out2), "fra", "segment", False, engine=engine, vocab=vocab,
                        emissions=(torch.cat([em, em[:1]]), np.concatenate([n_frames, n_frames[:1]])))       # (the orphan comes last and is left out)
    host = em.cpu().numpy()
    for k, name in enumerate(names):
        text_starred, tokens = ctc_segments.tokenize(texts[name], vocab, "segment", 32)
        want = CR.forced_align(host[k, :n_frames[k]], np.array([lab for word in tokens for lab in word], np.int32))
        assert want["status"] == CR.OK
        ref_rows = ctc_segments.align_words(want["path"], want["frame_score"], text_starred, tokens, 0, n_samples=len(clips[name]))
        got = grid_words(str(out2), name)
        expect = [(r["start"], r["end"] + (0.005 if r["start"] == r["end"] else 0.0), r["text"]) for r in ref_rows]
        assert [(float(repr(a)), float(repr(b)), t) for a, b, t in expect] == got
