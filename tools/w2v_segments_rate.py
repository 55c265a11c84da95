"""Device time of whisperX's emissions on the engine (pce_w2v_run_segments: the wav2vec2 forward pass over segments of unequal length, each
alone) beside the torch path's on the same device (Aligners/ctc_emissions.segment_emissions with the model in fp16: one forward per segment),
on random weights at the two published shapes: base (GroupNorm feature encoder, post-LN, 12 x 768) and large (LayerNorm feature encoder,
pre-LN, 24 x 1024).  Two batches of 256 segments cut from 32 clips of 30 s: seeded lengths uniform in 0.5 .. 12 s, and 5 s each (no slot is
longer than its segment).  Before anything is timed the device's emissions of the first segments are compared with segment_emissions in fp32 on
the same device (relative L2; more than 2 % ends the run).  Then the two paths alternate, twice each, so the spread is seen: the engine's call
between HIP events, five calls after a warm-up (a call returns when its emissions are complete); the torch path between HIP events too.
Per batch: both times, rows computed over rows valid, chunks and timed launch groups, the per-kernel shares (pce_profile_get).
Writes profiles/r21/w2v_segments_rate.txt, or the file named last (a comparison run keeps the record).
usage: w2v_segments_rate.py [segments [shapes [out]]]   (default 256 base,large profiles/r21/w2v_segments_rate.txt)"""
import os, sys
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
N_CLIPS, CLIP_S, CALLS, ROUNDS = 32, 30, 5, 2


def clip(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = 7000 * np.sin(2 * np.pi * 140.0 * t * (1 + 0.01 * t)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 1200 * rng.standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def batches(n_seg):
    """{name: [(clip, begin, end)]}: seeded, every segment inside its clip"""
    rng = np.random.default_rng(21)
    mixed, equal = [], []
    for k in range(n_seg):
        n = int(rng.uniform(0.5, 12.0) * 16000)
        b = int(rng.integers(0, CLIP_S * 16000 - n + 1))
        mixed.append((k % N_CLIPS, b, b + n))
        b5 = int(rng.integers(0, (CLIP_S - 5) * 16000 + 1))
        equal.append((k % N_CLIPS, b5, b5 + 5 * 16000))
    return {"0.5-12 s": mixed, "5 s": equal}


def torch_path(model, clips, segs, dev):
    """segment_emissions per clip, as whisperX.align calls it per file"""
    out = [None] * len(segs)
    for q in sorted({s[0] for s in segs}):
        mine = [k for k, s in enumerate(segs) if s[0] == q]
        em, n_frames = CE.segment_emissions(model, clips[q], [{"start": (segs[k][1] + 0.5) / 16000, "end": (segs[k][2] + 0.5) / 16000} for k in mine], dev)
        for r, k in enumerate(mine):
            out[k] = (em, r, int(n_frames[r]))
    return out


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


args = sys.argv[1:]
n_seg = int(args[0]) if args else 256
shapes = args[1].split(",") if len(args) > 1 else ["base", "large"]
out_path = os.path.abspath(args[2]) if len(args) > 2 else os.path.join(ROOT, "profiles", "r21", "w2v_segments_rate.txt")
out = []


def say(line=""):
    print(line, flush=True)
    out.append(line)


eng = pkg.ProsodyEngine(0)
dev = torch.device("cuda", eng.device)
clips = [clip(CLIP_S * 16000, 100 + i) for i in range(N_CLIPS)]
say(f"# tools/w2v_segments_rate.py: {n_seg} segments cut from {N_CLIPS} clips of {CLIP_S} s; random weights (torch.manual_seed(19)); "
    f"{'bf16' if eng._lib.pce_whisper_get_operands(eng._ctx) == 0 else 'fp16'} operands;")
say(f"# engine: w2v_segment_emissions, {CALLS} calls after a warm-up; torch: segment_emissions(model.half()), one forward per segment, one call; {ROUNDS} rounds, alternating")
for shape in shapes:
    torch.manual_seed(19)
    model = transformers.Wav2Vec2ForCTC(transformers.Wav2Vec2Config(**SHAPES[shape])).eval()
    eng.w2v_load(model)
    model = model.to(dev)
    eng.upload(clips, 16000)
    check = batches(n_seg)["0.5-12 s"][:8] + [(0, 100, 223), (1, 0, 400)]
    got = eng.w2v_segment_emissions(check).numpy()
    ref = torch_path(model, clips, check, dev)
    ref = [em[r, :n].cpu().numpy() for em, r, n in ref]
    assert [g.shape for g in got] == [r.shape for r in ref]
    dist = rel_l2(np.concatenate(got), np.concatenate(ref))
    say(f"{shape}: relative L2 distance to segment_emissions (fp32, same device) on {len(check)} segments: {dist:.3e}")
    if not dist < 0.02:
        sys.exit("the device's emissions are not close to the torch path's: nothing timed")
    half = model.half()
    for name, segs in batches(n_seg).items():
        eng.w2v_segment_emissions(segs)                          # allocations
        chunks, computed, valid = eng.w2v_segments_plan()
        torch_path(half, clips, segs[:8], dev)                   # warm-up
        e_ms, t_ms = [], []
        for _ in range(ROUNDS):
            e_ms.append(timed(lambda: eng.w2v_segment_emissions(segs), CALLS))
            t_ms.append(timed(lambda: torch_path(half, clips, segs, dev), 1))
        eng.profile_enable(True); eng.profile_reset()
        eng.w2v_segment_emissions(segs)
        eng.sync()
        prof = eng.profile(); eng.profile_enable(False)
        launches = sum(prof[k]["launches"] for k in prof if k != "w2v_forward")
        say(f"{shape}, {name}: {len(segs)} segments, {valid} frames")
        say(f"  engine  {'  '.join(f'{x:8.2f}' for x in e_ms)} ms per call     torch fp16  {'  '.join(f'{x:8.1f}' for x in t_ms)} ms per call   "
            f"(torch / engine, best of each: {min(t_ms) / min(e_ms):.1f} x)")
        say(f"  rows computed / rows valid: {computed} / {valid} = {computed / valid:.3f}   chunks {chunks}   timed launch groups {launches}")
        whole = prof["w2v_forward"]["total_ms"] if "w2v_forward" in prof else 0.0
        for k in STAGES:
            if k in prof and prof[k]["launches"]:
                ms = prof[k]["total_ms"]
                say(f"    {k:18s} {ms:9.3f} ms  {100 * ms / whole if whole and k != 'w2v_forward' else 100.0:5.1f} %  {prof[k]['launches']:5d} timed")
    del model, half
    torch.cuda.empty_cache()
eng.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w", encoding="utf-8") as fh:
    fh.write("\n".join(out) + "\n")
