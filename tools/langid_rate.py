"""Device time of Whisper language detection (pce_whisper_detect_language: one prefix pass over <|startoftranscript|> + k_lang_probs on the
language rows of the tied embedding) beside the only other way to the same answer: the same prefix step through pce_whisper_decode_step_ex with its
full logits projection (n x n_vocab x d) and k_decode_rules, every token that is no language token suppressed.  The two arg-max results are compared
before anything is timed.  Both calls are timed after the cross K / V of the batch exist (the first decoding call of a window computes them either
way).  usage: langid_rate.py [clips [model [runs]]]   (default 256 turbo 10; model: a whisper_weights.DIMS name)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import prosody_control_french_tts_amd as pkg
from prosody_control_french_tts_amd import synth, whisper_weights as WW

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
model = sys.argv[2] if len(sys.argv) > 2 else "turbo"
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 10
edims, tdims = WW.DIMS[model], WW.TEXT_DIMS[model]
V = tdims["n_vocab"]
n_lang = 100 if V == 51866 else 99
eot, sot = 50257, 50258
lang_begin, ts_begin = sot + 1, 50364 + (n_lang - 99)
eng = pkg.ProsodyEngine(0)
eng.upload(synth.synth_batch(n, 10.0, 16000, first=0), 16000)
eng.logmel_run(edims["n_mels"])
eng.whisper_load(edims, WW.pack(WW.synthetic_weights(edims), edims))
eng.whisper_decoder_load(tdims, WW.pack_decoder(WW.greedy_test_decoder_weights(tdims), tdims))
eng.whisper_encode_run()
# the full-projection way: every id outside the language range suppressed (bit 0), sample_begin 1 on the one-token prompt (no timestamp rule bites:
# max_initial_timestamp None, and the first-position rule only removes what the mask already has)
mask = np.ones(V, dtype=np.uint8); mask[lang_begin:lang_begin + n_lang] = 0
prompts = [[sot]] * n


def full():
    return eng.whisper_decode_step_ex(prompts, 1, eot, ts_begin, mask, None, no_cache=True)[0]


ids, probs = eng.whisper_detect_language(sot, lang_begin, n_lang)
want = full()
if not np.array_equal(ids, want):
    sys.exit(f"arg-max differs between the two paths for {int(np.sum(ids != want))} of {n} clips: nothing timed")
eng.profile_enable(True)
for name, fn in (("detect_language (n_lang rows)", lambda: eng.whisper_detect_language(sot, lang_begin, n_lang)), ("prefix step, full projection", full)):
    fn(); eng.sync(); eng.profile_reset()
    t0 = time.perf_counter()
    for _ in range(runs):
        fn()
    eng.sync()
    wall = (time.perf_counter() - t0) / runs * 1e3
    dev = eng.profile()["whisper_decode_step"]["total_ms"] / runs
    print(f"{name:32s} {dev:8.3f} ms device per call   {wall:8.3f} ms wall (upload + sync + results included)")
d = tdims["n_state"]
print(f"{n} clips, model {model}: d = {d}, n_vocab = {V}, n_lang = {n_lang}; projection rows {V} -> {n_lang}; logits the full path fetches from: "
      f"{n * V * 4 / 1e6:.1f} MB, results of detect_language: {n * (n_lang + 1) * 4 / 1e3:.1f} kB")
eng.close()
