"""Device time of the wav2vec2 / MMS CTC forward pass (pce_w2v_run) per stage, beside the torch path's time on the same device
(Aligners/ctc_emissions.hf_emissions: the caller's transformers model, batches of four windows), on random weights at the two published shapes:
base (GroupNorm feature encoder, post-LN, 12 x 768) and large (LayerNorm feature encoder, pre-LN, 24 x 1024).  64 clips of 30 s at the default
(30 s, 2 s) windows.  Before anything is timed the device's emissions of the first clips are compared with hf_emissions in fp32 on the same
device (relative L2; more than 2 % ends the run).  HIP events via the engine's profiler; the torch path by wall clock around a synchronised call.
Writes profiles/r19/w2v_rate.txt, or the file named last (a comparison run keeps the record).
usage: w2v_rate.py [clips [runs [shapes [out]]]]   (default 64 2 base,large profiles/r19/w2v_rate.txt)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch                                                   # (before libpce.so: one HIP runtime for both)
import transformers
import prosody_control_french_tts_amd as pkg
from prosody_control_french_tts_amd.Aligners import ctc_emissions as CE

SHAPES = {
    "base": dict(vocab_size=32),
    "large": dict(vocab_size=32, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, feat_extract_norm="layer",
                  conv_bias=True, do_stable_layer_norm=True),
}
STAGES = ["k_w2v_wave", "k_gemm_bf16", "k_gemm_wide", "k_layernorm", "k_attention_lean", "k_w2v_posconv", "k_w2v_tail", "w2v_forward"]


def clip(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = 7000 * np.sin(2 * np.pi * 140.0 * t * (1 + 0.01 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 1200 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


args = sys.argv[1:]
n_clips, runs = int(args[0]) if args else 64, int(args[1]) if len(args) > 1 else 2
shapes = args[2].split(",") if len(args) > 2 else ["base", "large"]
out_path = os.path.abspath(args[3]) if len(args) > 3 else os.path.join(ROOT, "profiles", "r19", "w2v_rate.txt")
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


eng = pkg.ProsodyEngine(0)
dev = torch.device("cuda", eng.device)
clips = [clip(30 * 16000, 100 + i) for i in range(n_clips)]
say(f"# tools/w2v_rate.py: {n_clips} clips of 30 s, windows (30 s, 2 s): {n_clips} windows of 544 000 samples -> 1 699 frames each, 1 500 kept;")
say(f"# random weights (torch.manual_seed(19)); {'bf16' if eng._lib.pce_whisper_get_operands(eng._ctx) == 0 else 'fp16'} operands; {runs} timed runs each")
for shape in shapes:
    torch.manual_seed(19)
    model = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**SHAPES[shape])).eval()
    eng.w2v_load(model)
    model = model.to(dev)
    n_check = min(2, n_clips)
    eng.upload(clips[:n_check], 16000)
    got = eng.w2v_emissions().numpy()
    ref, n_frames = CE.hf_emissions(model, clips[:n_check], dev)
    ref = ref.cpu().numpy()
    dist = rel_l2(np.concatenate(got), np.concatenate([ref[i, :n_frames[i]] for i in range(n_check)]))
    say(f"{shape}: relative L2 distance to hf_emissions (fp32, same device) on {n_check} clips: {dist:.3e}")
    if not dist < 0.02:
        sys.exit("the device's emissions are not close to the torch path's: nothing timed")
    eng.upload(clips, 16000)
    eng.w2v_emissions()                                         # allocations
    eng.profile_enable(True); eng.profile_reset()
    t0 = time.perf_counter()
    for _ in range(runs):
        eng.w2v_emissions()
    wall = (time.perf_counter() - t0) / runs * 1e3
    prof = eng.profile(); eng.profile_enable(False)
    for k in STAGES:
        if k in prof and prof[k]["launches"]:
            ms, fl = prof[k]["total_ms"] / runs, prof[k]["flops"] / runs
            rate = f"{fl / ms / 1e9:8.1f} TFLOP/s" if fl else ""
            say(f"  {k:18s} {ms:10.2f} ms per run  {prof[k]['launches'] // runs:6d} launches  {rate}")
    say(f"  whole call (w2v_emissions, emissions left on the device): {wall:.1f} ms for {n_clips} clips = {wall / n_clips:.2f} ms per 30 s clip")
    for name in ("fp32", "fp16"):
        m = model if name == "fp32" else model.half()            # (half() converts in place: fp32 is timed first, on the untouched model)
        assert next(m.parameters()).dtype == (torch.float32 if name == "fp32" else torch.float16)
        CE.hf_emissions(m, clips[:4], dev)                       # warm-up
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        CE.hf_emissions(m, clips, dev)
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3
        say(f"  torch path (hf_emissions, model in {name}, batches of 4 windows): {ms:.1f} ms = {ms / n_clips:.2f} ms per clip  ({ms / wall:.2f} x the engine's call)")
    del model
    torch.cuda.empty_cache()
eng.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w", encoding="utf-8") as fh:
    fh.write("\n".join(out) + "\n")
