"""The residual epilogue of the persistent 256 x 256 GEMM (FEPI_RESID, csrc/pce_gemm256.inc) and the encoder path built on it.

Everything here is bit for bit: the epilogue computes r16(resid + r16(acc + bias)), the same two roundings k_add_layernorm makes from a stored
branch output, so the plain epilogue's result plus one 16-bit add is the reference, and the fused encoder must return the bytes of the unfused one
(a context created with PCE_RESID_EPILOGUE=0)."""
import os

import numpy as np
import pytest
import torch

from prosody_control_french_tts_amd import synth, whisper_weights as WW

pytestmark = pytest.mark.gpu

# (M, N, K): a ragged last row tile with a one-step K loop (its own wait path) | nk = 2: both waits that follow an epilogue fall into one tile pair |
# the attention projection of one clip | 270 tiles on 256 workgroups: some run a second tile after an epilogue | Whisper-medium's fc2
SHAPES = [(300, 256, 64), (300, 768, 128), (1500, 768, 768), (23040, 768, 768), (1500, 1024, 4096)]
BIG = (23040, 768, 768)

_inputs, _results = {}, {}


def _bits(x, dtype):
    """float32 array -> uint16 bit patterns of the 16-bit type (round to nearest even)"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).view(torch.int16).numpy().view(np.uint16)


def _f32(b, dtype):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16)).view(dtype).float().numpy()


def _problem(shape):
    """A, B, bias and the residual values of a shape (float32; the residual as Whisper's stream has it: around +-8 with outliers of +-2 000, so the
    second rounding happens at several exponents)"""
    if shape not in _inputs:
        M, N, K = shape
        rng = np.random.default_rng(M * 31 + N * 7 + K)
        A = rng.standard_normal((M, K), dtype=np.float32)
        B = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32)
        R = rng.standard_normal((M, N), dtype=np.float32) * 8.0
        out = rng.random((M, N)) < 0.01
        R[out] = (np.sign(R[out]) * rng.uniform(500.0, 2000.0, size=int(out.sum()))).astype(np.float32)
        _inputs[shape] = (A, B, bias, R)
    return _inputs[shape]


def _fused(engine, shape, name, dtype):
    """the in-place result of a shape on the engine's current operand type (computed once per type)"""
    if (shape, name) not in _results:
        A, B, bias, R = _problem(shape)
        _results[(shape, name)] = engine.selftest_gemm_resid(A, B, bias, _bits(R, dtype))
    return _results[(shape, name)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_residual_epilogue_equals_plain_epilogue_plus_add(engine, ops, shape):
    dtype = getattr(torch, ops["torch"])
    A, B, bias, R = _problem(shape)
    got = _fused(engine, shape, ops["name"], dtype)
    delta = engine.selftest_gemm(A, B, bias, 0)                       # r16(acc + bias), decoded to float32
    want = _bits(_f32(_bits(R, dtype), dtype) + delta, dtype)        # the sum of two 16-bit values is exact in float32 up to its one rounding
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    print(f"{ops['name']} {shape}: {bad.size} of {want.size} elements differ")
    assert np.array_equal(got, want), (shape, ops["name"], bad[:8].tolist())


def test_residual_epilogue_is_deterministic_and_row_count_independent(engine):
    """rows 0-255 of the 23 040-row product (another tile order, other workgroups, second tiles after an epilogue) are the bits of the same rows run
    alone with M = 256, and a repeat gives the same bits: the rule of test_persistent_256_gemm_is_deterministic_and_row_count_independent"""
    name = engine.whisper_operands                                   # whatever operand type this run of the suite selected
    dtype = torch.bfloat16 if name == "bf16" else torch.float16
    A, B, bias, R = _problem(BIG)
    big = _fused(engine, BIG, name, dtype)
    small = engine.selftest_gemm_resid(A[:256], B, bias, _bits(R[:256], dtype))
    assert np.array_equal(big[:256], small)
    assert np.array_equal(engine.selftest_gemm_resid(A, B, bias, _bits(R, dtype)), big)


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


@pytest.fixture(scope="module")
def engines():
    """the test's own contexts: the product's default (residual adds in both GEMM epilogues), the stored-branch-output path, and the A/B mode
    that fuses fc2 only"""
    made = [_fresh_engine(PCE_RESID_EPILOGUE=v) for v in ("1", "0", "2")]
    for e in made:
        e.whisper_set_operands("fp16-resid16")
    yield made
    for e in made:
        e.close()


def _clips(n):
    return [synth.synth_clip(70 + i, seconds=10.0) for i in range(n)]


def _encode(eng, dims, clips):
    W = WW.synthetic_weights(dims, seed=dims["n_state"] + dims["n_layer"])
    eng.upload(clips, 16000); eng.logmel_run(dims["n_mels"])
    eng.whisper_load(dims, WW.pack(W, dims)); eng.whisper_encode_run()
    return [eng.whisper_encode_fetch(i) for i in range(len(clips))]


@pytest.mark.parametrize("model,layers", [("small", 2), ("base", 2), ("medium", 1)])
def test_fused_encoder_returns_the_bytes_of_the_unfused_one(engines, model, layers):
    """small: the bench's width; base: N = 2 tiles; medium: N = 4 tiles (another tile walk of both GEMMs); one layer also makes the pass after fc2
    the ln_post form"""
    fused, plain, fc2_only = engines
    dims = dict(WW.DIMS[model], n_layer=layers)
    clips = _clips(2)
    a, b, c = _encode(fused, dims, clips), _encode(plain, dims, clips), _encode(fc2_only, dims, clips)
    for i in range(2):
        assert np.isfinite(a[i]).all() and float(np.std(a[i])) > 0.1
        assert a[i].tobytes() == b[i].tobytes(), (model, i, int(np.count_nonzero(a[i] != b[i])))
        assert c[i].tobytes() == b[i].tobytes(), (model, i, int(np.count_nonzero(c[i] != b[i])))


def test_fused_encoder_is_batch_independent(engines):
    fused = engines[0]
    dims = dict(WW.DIMS["small"], n_layer=2)
    clips = _clips(3)
    alone, batch = _encode(fused, dims, clips[:1]), _encode(fused, dims, clips)
    assert alone[0].tobytes() == batch[0].tobytes()
