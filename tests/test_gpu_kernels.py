"""Kernel-level checks of the tiled / few-row GEMMs (k_gemm_skinny, k_gemm_wide, k_gemm_bf16 in its two- and four-stage forms) and the LayerNorm
kernels (k_layernorm, the six k_add_layernorm forms) through the product's own launch code (pce_selftest_gemm_tiled, pce_selftest_layernorm), and the
models past d = 1280 end to end.

References are float64 restatements of the ROUNDED operands.  Bounds are derived per element, not fitted:
  * one rounding of a 16-bit output: 2^-8 (bf16) / 2^-11 (fp16) of its magnitude;
  * fp32 accumulation: K 2^-24 sum |a b| (plus one fp32 rounding per later addition);
  * GELU: the Abramowitz-Stegun erf error (1.5e-7) times |x| / 2, the fp32 steps of the polynomial, and the input error times the GELU slope (<= 1.13);
  * LayerNorm: the fp32 sums of the two passes (terms per lane + the 6-level wave tree), rsqrt within 2 ulp."""
import os

import numpy as np
import pytest
import torch

from oracle import bert_oracle as BO
from oracle import whisper_oracle as WO
from prosody_control_french_tts_amd import PceError, bert_weights as BW, synth, whisper_weights as WW
from tests.gemm_restatement import (U, _check16, _check32, _dt, _gelu, _gelu_err, _half_ulp, _ln_ref, bits, gemm_acc, gemm_pre, r16, resid_err,  # noqa: F401
                                    val)

pytestmark = pytest.mark.gpu

EPI_BF16, EPI_GELU, EPI_GELU_POS, EPI_RESID, EPI_QKV, EPI_F32 = range(6)
AUTO, SKINNY, WIDE, T128, T128_DEEP = range(5)
torch.set_num_threads(min(16, torch.get_num_threads()))


class Prob:
    """One random GEMM problem: rounded operands (uint16 bits + float64 values), bias, float64 products for the rows checked."""

    def __init__(self, ops, M, N, K, seed, rows=None):
        rng = np.random.default_rng(seed)
        self.M, self.N, self.K, self.ops = M, N, K, ops
        self.a = bits(rng.standard_normal((M, K)), ops)
        self.b = bits(rng.standard_normal((N, K)) / np.sqrt(K), ops)
        self.bias = rng.standard_normal(N).astype(np.float32)
        # rows checked against float64: all of a small problem; of a big one the tile and clip edges and a random sample
        if rows is None:
            rows = np.arange(M) if M <= 600 else np.unique(np.r_[0, 1, 126, 127, 128, 129, 1499, 1500, 1501, 2999, 3000, M - 1,
                                                                rng.integers(0, M, 48)].clip(0, M - 1))
        self.rows = rows
        A, B = val(self.a, ops)[rows], val(self.b, ops)
        self.acc, self.mag, self.acc_err = gemm_acc(A, B)          # (mag: sum |a b|)

    def run(self, eng, epi, kernel, C=None, **kw):
        f32 = epi in (EPI_GELU_POS, EPI_RESID, EPI_F32)
        if C is None:
            C = np.zeros(self.M * self.N, dtype=np.float32 if f32 else np.uint16)
        used = eng.selftest_gemm_tiled(epi, self.a.ravel(), self.b.ravel(), self.bias, self.M, self.N, self.K, C, lda=self.K,
                                       ldc=kw.pop("ldc", self.N), kernel=kernel, **kw)
        return C.reshape(self.M, -1), used

    def check(self, epi, C, what, old=None):
        pre, err = gemm_pre(self.acc, self.acc_err, self.bias)
        got = C[self.rows]
        if epi == EPI_BF16 or epi == EPI_QKV:
            _check16(got, pre, err, self.ops, what)
        elif epi == EPI_GELU:
            _check16(got, _gelu(pre), _gelu_err(pre, err), self.ops, what)
        elif epi == EPI_RESID:
            o = old[self.rows].astype(np.float64)
            _check32(got, o + pre, resid_err(o, self.acc, err), what)
        else:
            _check32(got, pre, err, what)


WIDTHS = (384, 512, 768, 1024, 1280)


def _fits(kernel, epi, M, N, K, batch=1):
    if kernel == SKINNY:
        return epi in (EPI_BF16, EPI_GELU, EPI_RESID) and batch == 1 and M <= 1024 and N <= 4096 and N % 32 == 0 and K % 256 == 0
    if kernel == WIDE:
        return N % 256 == 0 and K % 32 == 0
    return N % 128 == 0 and K % 64 == 0


@pytest.mark.parametrize("d", WIDTHS)
def test_tiled_gemms_at_model_widths(engine, ops, d):
    """Every kernel x the projections of a d-wide layer (N = d, K = 4 d: fc2 / out-projection; N = 4 d, K = d: fc1) at ragged M; a kernel that cannot
    compute a shape (k_gemm_wide at N % 256 != 0, the few-row kernel past N = 4096) is refused with PCE_E_LIMIT, never launched."""
    cases = [(EPI_BF16, 129, d, 4 * d), (EPI_GELU, 127, 4 * d, d), (EPI_RESID, 1, d, 4 * d)]
    for ci, (epi, M, N, K) in enumerate(cases):
        p = Prob(ops, M, N, K, seed=d * 10 + ci)
        for kernel in (SKINNY, WIDE, T128, T128_DEEP):
            old = np.random.default_rng(ci).standard_normal(M * N).astype(np.float32) if epi == EPI_RESID else None
            if not _fits(kernel, epi, M, N, K):
                with pytest.raises(PceError, match="status -5"):
                    p.run(engine, epi, kernel, C=old)
                continue
            C, used = p.run(engine, epi, kernel, C=None if old is None else old.copy())
            assert used == kernel
            p.check(epi, C, (ops["name"], d, epi, kernel), old=None if old is None else old.reshape(M, N))


def test_bias_and_fp32_epilogues_are_identical_across_kernels_and_row_counts(engine, ops):
    """pce_whisper_impl.inc (gemm_choose) claims the bias and fp32-accumulate epilogues give the same bits on the few-row, 128 x 256 and 128 x 128 kernels (the
    sums run in the same order), and EPI_F32 the same bits on 128 x 256 and the four-stage kernel; and a row's bits never depend on M."""
    M, N, K = 300, 1536, 768
    p = Prob(ops, M, N, K, seed=5)
    old = np.random.default_rng(6).standard_normal(M * N).astype(np.float32)
    for epi in (EPI_BF16, EPI_RESID):
        outs = {k: p.run(engine, epi, k, C=None if epi == EPI_BF16 else old.copy())[0] for k in (SKINNY, WIDE, T128, T128_DEEP)}
        p.check(epi, outs[WIDE], (ops["name"], epi), old=old.reshape(M, N))
        for k in (SKINNY, T128, T128_DEEP):
            assert np.array_equal(outs[k], outs[WIDE]), (ops["name"], epi, k)
        # the first rows alone (one tile, one row) and inside a taller problem
        for m in (1, 129):
            q = Prob(ops, m, N, K, seed=0, rows=np.arange(0))
            q.a, q.b, q.bias = p.a[:m].copy(), p.b, p.bias
            for k in (SKINNY, WIDE, T128, T128_DEEP):
                c = q.run(engine, epi, k, C=None if epi == EPI_BF16 else old[:m * N].copy())[0]
                assert np.array_equal(c, outs[WIDE][:m]), (ops["name"], epi, k, m)
    f = {k: p.run(engine, EPI_F32, k)[0] for k in (WIDE, T128_DEEP, T128)}
    p.check(EPI_F32, f[WIDE], (ops["name"], "f32"))
    assert np.array_equal(f[WIDE], f[T128_DEEP]) and np.array_equal(f[WIDE], f[T128])


def test_vocabulary_logits_and_bert_classifier(engine, ops):
    """EPI_F32 as the decoding step runs it (N = 51 968: M = 3 on the four-stage kernel, M = 1 100 on 128 x 256, bit-identical to each other) and as
    BERT's classifier (N = 128)."""
    N, K = 51968, 384
    p = Prob(ops, 1100, N, K, seed=7, rows=np.r_[0:3, 127:130, 1096:1100])
    C, used = p.run(engine, EPI_F32, AUTO)
    assert used == WIDE
    p.check(EPI_F32, C, (ops["name"], "logits 1100"))
    C4, _ = p.run(engine, EPI_F32, T128_DEEP)
    assert np.array_equal(C, C4)
    q = Prob(ops, 3, N, K, seed=0, rows=np.arange(0))
    q.a, q.b, q.bias = p.a[:3].copy(), p.b, p.bias
    c3, used = q.run(engine, EPI_F32, AUTO)
    assert used == T128_DEEP and np.array_equal(c3, C[:3])
    cls = Prob(ops, 37, 128, 768, seed=8)
    for k in (AUTO, T128):
        C, used = cls.run(engine, EPI_F32, k)
        assert used in (T128, T128_DEEP)
        cls.check(EPI_F32, C, (ops["name"], "classifier", k))


@pytest.mark.parametrize("S,M,vt_sp", [(1500, 4500, 1536), (48, 3 * 48 - 20, 64)])
def test_qkv_epilogue_writes_the_v_image_and_nothing_else(engine, ops, S, M, vt_sp):
    """EPI_QKV: Q | K row-major, V transposed per clip (clip boundaries inside a 128-row tile: 1 500 = 11 x 128 + 92, 48 rows), for the encoder's
    S = 1 500 and a short teacher-forced T_pad; the key padding t >= S of every clip and every byte past the image keep their sentinel."""
    d = 512
    N, K, v0 = 3 * d, d, 2 * d
    p = Prob(ops, M, N, K, seed=S)
    nclip = -(-M // S)
    for kernel in (WIDE, T128, T128_DEEP):
        sentinel = np.uint16(0x7FFF)                          # a NaN in both 16-bit types: no finite product rounds to it
        vt = np.full(nclip * d * vt_sp + 512, sentinel, dtype=np.uint16)
        C = np.zeros(M * v0, dtype=np.uint16)
        C, used = p.run(engine, EPI_QKV, kernel, C=C, ldc=v0, v_col0=v0, rows_per_clip=S, vt=vt, vt_sp=vt_sp)
        assert used == kernel
        pre = p.acc + p.bias.astype(np.float64)
        err = p.acc_err + U * np.abs(pre)
        _check16(C[p.rows], pre[:, :v0], err[:, :v0], ops, (ops["name"], "qk", kernel))
        img = vt[:nclip * d * vt_sp].reshape(nclip, d, vt_sp)
        clip, t = p.rows // S, p.rows % S
        _check16(img[clip, :, t], pre[:, v0:], err[:, v0:], ops, (ops["name"], "v", kernel))
        written = np.zeros((nclip, vt_sp), dtype=bool)
        written[np.arange(M) // S, np.arange(M) % S] = True
        assert (img.transpose(0, 2, 1)[~written] == sentinel).all(), (ops["name"], kernel)
        assert (img.transpose(0, 2, 1)[written] != sentinel).all()
        assert (vt[nclip * d * vt_sp:] == sentinel).all()


@pytest.mark.parametrize("d", [384, 512])
def test_convolution_stem_forms(engine, ops, d):
    """The encoder's two convolutions as launch_gemm runs them: batch 2, overlapping A rows (lda < K), conv1 GELU to 16 bits, conv2 GELU + the
    positional table (pos_T = 1 500) in fp32; the reference builds the im2col explicitly."""
    nm, F, T = 80, 3000, 1500
    rng = np.random.default_rng(d)
    K1p = -(-3 * nm // 64) * 64
    mel = np.zeros((2, F + 2, nm), dtype=np.float32)
    mel[:, 1:F + 1] = rng.standard_normal((2, F, nm))
    a1 = np.concatenate([bits(mel, ops).ravel(), np.zeros(K1p, np.uint16)])          # (the last row's K1p - 3 nm zero-weight columns read past it)
    w1 = np.zeros((d, K1p), dtype=np.float32)
    w1[:, :3 * nm] = rng.standard_normal((d, 3 * nm)) / np.sqrt(3 * nm)
    b1 = rng.standard_normal(d).astype(np.float32)
    c1 = np.zeros(2 * (F + 2) * d, dtype=np.uint16)
    w2 = rng.standard_normal((d, 3 * d)) / np.sqrt(3 * d)
    b2 = rng.standard_normal(d).astype(np.float32)
    pos = np.asarray(WO.sinusoids(T, d), dtype=np.float32)
    Av, W1v = val(a1, ops), val(bits(w1, ops), ops)
    for kernel in (AUTO, WIDE, T128, T128_DEEP):
        if not _fits(kernel, EPI_GELU, F, d, K1p) or not _fits(kernel, EPI_GELU_POS, T, d, 3 * d):
            continue
        c1[:] = 0
        # (C is one buffer: conv1's output rows start one padded row in, as in pce_whisper_encode_run -- the self-test writes from C[0], so the
        #  padded image is assembled from its result)
        out1 = np.zeros(2 * (F + 2) * d - d, dtype=np.uint16)
        engine.selftest_gemm_tiled(EPI_GELU, a1, bits(w1, ops).ravel(), b1, F, d, K1p, out1, lda=nm, ldc=d, kernel=kernel, a_batch=(F + 2) * nm,
                                   batch=2, c_batch=(F + 2) * d)
        c1[d:] = out1
        img = c1.reshape(2, F + 2, d)
        for bi in range(2):
            rows = np.r_[0:3, 1498:1502, F - 3:F]
            cols = Av[bi * (F + 2) * nm + rows[:, None] * nm + np.arange(K1p)[None, :]]          # im2col: row t = padded rows t .. t + 2
            pre = cols @ W1v.T + b1
            err = K1p * U * (np.abs(cols) @ np.abs(W1v).T) + U * np.abs(pre)
            _check16(img[bi, 1 + rows], _gelu(pre), _gelu_err(pre, err), ops, (ops["name"], "conv1", kernel, bi))
        assert (img[:, 0] == 0).all() and (img[:, F + 1] == 0).all()
        a2 = c1.copy()
        w2b = bits(w2, ops)
        out2 = np.zeros(2 * T * d, dtype=np.float32)
        used = engine.selftest_gemm_tiled(EPI_GELU_POS, a2, w2b.ravel(), b2, T, d, 3 * d, out2, lda=2 * d, ldc=d, kernel=kernel,
                                          a_batch=(F + 2) * d, batch=2, c_batch=T * d, pos=pos)
        A2, W2v = val(a2, ops), val(w2b, ops)
        o2 = out2.reshape(2, T, d)
        for bi in range(2):
            rows = np.r_[0:3, 126:130, 700, T - 2:T]
            cols = A2[bi * (F + 2) * d + rows[:, None] * 2 * d + np.arange(3 * d)[None, :]]      # stride 2: padded rows 2t .. 2t + 2
            pre = cols @ W2v.T + b2
            err = _gelu_err(pre, 3 * d * U * (np.abs(cols) @ np.abs(W2v).T) + U * np.abs(pre))
            want = _gelu(pre) + pos[rows]
            _check32(o2[bi, rows], want, err + U * np.abs(pos[rows]), (ops["name"], "conv2", kernel, used, bi))


def test_tiled_gemm_refuses_what_it_cannot_compute(engine):
    """The self-test checks every extent a launch can address and every shape condition before it allocates: K tails (k_gemm_bf16 walks K / 64
    steps), N % 128, the few-row conditions, short buffers."""
    ops = dict(torch="float16")
    a, b = np.zeros(129 * 256, np.uint16), np.zeros(256 * 256, np.uint16)
    C = np.zeros(129 * 256, np.uint16)
    for kernel, (M, N, K) in [(T128, (129, 256, 160)), (T128_DEEP, (129, 256, 96)), (WIDE, (129, 128, 64)), (SKINNY, (129, 256, 128)),
                              (SKINNY, (129, 200, 256)), (AUTO, (129, 200, 64))]:
        with pytest.raises(PceError, match="status -5"):
            engine.selftest_gemm_tiled(EPI_BF16, a[:M * K], b[:N * K], None, M, N, K, np.zeros(M * N, np.uint16), lda=K, ldc=N, kernel=kernel)
    with pytest.raises(PceError, match="status -1"):                      # A one element short
        engine.selftest_gemm_tiled(EPI_BF16, a[:129 * 64 - 1], b[:256 * 64], None, 129, 256, 64, C, lda=64, ldc=256, kernel=T128)
    with pytest.raises(PceError, match="status -1"):                      # C one row short
        engine.selftest_gemm_tiled(EPI_BF16, a[:129 * 64], b[:256 * 64], None, 129, 256, 64, C[:128 * 256], lda=64, ldc=256, kernel=T128)
    with pytest.raises(PceError, match="status -1"):                      # V image one clip short
        engine.selftest_gemm_tiled(EPI_QKV, a[:129 * 64], b[:256 * 64], None, 129, 256, 64, C, lda=64, ldc=128, kernel=T128, v_col0=128,
                                   rows_per_clip=64, vt=np.zeros(2 * 128 * 64, np.uint16), vt_sp=64)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
LN_WIDTHS = (128, 384, 1280, 1536, 2048)


def _ln_rows(d, n_random, rng, spread=1.0):
    """random rows + the edge rows: a constant row (variance 0), a large mean with a small spread (the two-pass statistics), a tiny spread
    against eps"""
    x = rng.standard_normal((n_random, d)) * spread
    edge = np.stack([np.full(d, 0.75), 1000.0 + rng.standard_normal(d), 3.0 + 1e-3 * rng.standard_normal(d)])
    return np.concatenate([x, edge]).astype(np.float32)


@pytest.mark.parametrize("d", LN_WIDTHS)
def test_layernorm_against_float64(engine, ops, d):
    """k_layernorm to fp32 and to 16 bits (with round_in16 and the in-place fp32 copy the BERT layers keep) at d = 128 (half the lanes idle), 384,
    1280 (five float4 per lane), 1536 and 2048 (the eight-float4 form); rows = 1, 3 and 4 097 plus the edge rows."""
    rng = np.random.default_rng(d)
    w = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    eps = 1e-5
    for n in (1, 3, 4097):
        x = _ln_rows(d, n, rng)
        y, err = _ln_ref(x, w, b, eps)
        out, _, _ = engine.selftest_layernorm(0, x, w, b, eps)
        _check32(out, y, err, (ops["name"], d, n, "fp32"))
        out16, res, _ = engine.selftest_layernorm(1, x, w, b, eps, flags=2)
        _check32(res, y, err, (ops["name"], d, n, "out2"))
        assert np.array_equal(out16, bits(res, ops)), (ops["name"], d, n)          # the 16-bit output is the fp32 value rounded once
    xr = r16(x, ops)
    y, err = _ln_ref(xr, w, b, eps)
    out16, _, _ = engine.selftest_layernorm(1, x, w, b, eps, flags=1)
    _check16(out16, y, err, ops, (ops["name"], d, "round_in16"))


@pytest.mark.parametrize("d", LN_WIDTHS)
def test_add_layernorm_forms_against_float64(engine, ops, d):
    """The six k_add_layernorm forms (fp32 / 16-bit output x fp32 stream, fp32 in / 16-bit stream out, 16-bit stream), with and without delta2,
    write_resid and the 16-bit copy: the stream they write is the EXACT rounding sequence r16(r16(x + delta) + delta2) (fp32 sums, each rounded to
    the stream's type), the output its LayerNorm within the derived bound."""
    rng = np.random.default_rng(d + 1)
    w = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    b = (0.1 * rng.standard_normal(d)).astype(np.float32)
    eps = 1e-5
    x = _ln_rows(d, 5, rng)
    n = x.shape[0]
    dl = bits(0.5 * rng.standard_normal((n, d)), ops)
    dl2 = bits(0.5 * rng.standard_normal((n, d)), ops)
    f = lambda u: val(u, ops).astype(np.float32)
    for o in (0, 1):
        for st in (0, 1, 2):
            form = 2 + 3 * o + st
            xin = bits(x, ops) if st == 2 else x
            for with2 in (False, True):
                for wr in (0, 1):
                    out, res, cp = engine.selftest_layernorm(form, xin, w, b, eps, flags=4 * wr, delta=dl, delta2=dl2 if with2 else None,
                                                             want_copy=o == 0)
                    # the restatement: fp32 additions, rounded to the stream type after each where the stream is 16-bit
                    rs = (lambda z: r16(z, ops)) if st else (lambda z: z)
                    v = rs(f(xin) if st == 2 else x)
                    v = rs(np.float32(v) + f(dl))
                    if with2:
                        v = rs(np.float32(v) + f(dl2))
                    what = (ops["name"], d, form, with2, wr)
                    if st == 0:
                        assert np.array_equal(res, v if wr else x), what
                    elif st == 1:
                        assert np.array_equal(res, bits(v, ops) if wr else np.zeros_like(res)), what
                    else:
                        assert np.array_equal(res, bits(v, ops) if wr else xin), what
                    y, err = _ln_ref(v, w, b, eps)
                    if o == 0:
                        _check32(out, y, err, what)
                        assert np.array_equal(cp, bits(out, ops)), what
                    else:
                        _check16(out, y, err, ops, what)


# ---------------------------------------------------------------------------------------------------------------
# end to end past d = 1280
# ---------------------------------------------------------------------------------------------------------------
def _fresh_engine(**env):
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


def _encoder_decoder_end_to_end(eng, d, heads, ops_name):
    """a 1-layer encoder and a 2-layer decoder of the given width: encoder output, the teacher-forced alignment cost and free-running greedy tokens
    and log-probabilities against the restatement (the bounds of tests/test_gpu_whisper.py and tests/test_gpu_whisper_large.py)"""
    from tests.test_whisper_hf_crosscheck import _greedy_gold
    from prosody_control_french_tts_amd.Aligners import decoding as DEC
    g, rules = _greedy_gold()
    init = g["initial"].tolist()
    edims = dict(n_mels=80, n_ctx=1500, n_state=d, n_head=heads, n_layer=1)
    tdims = dict(n_vocab=300, n_text_ctx=96, n_state=d, n_head=heads, n_layer=2)
    We, Wd = WW.synthetic_weights(edims, seed=d), WW.greedy_test_decoder_weights(tdims, seed=d + 1)
    clips = [synth.synth_clip(60, seconds=4.0), synth.synth_clip(61, seconds=2.5)]
    eng.whisper_set_operands(ops_name)
    eng.upload(clips, 16000); eng.logmel_run(80)
    eng.whisper_load(edims, WW.pack(We, edims)); eng.whisper_encode_run()
    eng.whisper_decoder_load(tdims, WW.pack_decoder(Wd, tdims))
    from tests.conftest import OPERANDS
    bounds = OPERANDS[ops_name]
    encs = []
    for i, c in enumerate(clips):
        got = eng.whisper_encode_fetch(i)
        want = WO.encoder_forward(WO.log_mel(c, 80), We, edims)
        rel = np.linalg.norm(got - want) / np.linalg.norm(want)
        assert rel <= bounds["enc_l2"], (d, ops_name, i, rel)
        assert np.max(np.abs(got - want)) / max(1.0, float(np.std(want))) <= bounds["enc_max"], (d, ops_name, i)
        encs.append(got)
    rng = np.random.default_rng(d)
    toks = [rng.integers(0, 300, size=n).tolist() for n in (21, 34)]
    num_frames = [len(c) // 160 for c in clips]
    res = eng.whisper_align(toks, num_frames, 3, want_cost=True)
    for i in range(2):
        cost, _, _ = WO.find_alignment(toks[i], encs[i], Wd, tdims, num_frames[i], 3)
        assert res[i]["cost"].shape == cost.shape
        assert np.max(np.abs(res[i]["cost"] - cost)) <= 0.08, (d, ops_name, i)
        assert np.linalg.norm(res[i]["cost"] - cost) / np.linalg.norm(cost) <= 3e-2
    out, lps, _ = DEC.decode_batch(eng, tdims["n_vocab"], [list(init)] * 2, [len(init)] * 2, rules, sample_len=8)
    for i in range(2):
        want = WO.greedy_decode(encs[i], Wd, tdims, init, rules, sample_len=8)[len(init):]
        got = out[i]
        agree = next((k for k, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
        assert agree >= 3, (d, ops_name, i, got, want)
        seq = list(init)
        for k in range(agree):
            logits = WO.find_alignment(seq, encs[i], Wd, tdims, 2, 0, want_internal=True)["logits"][-1]
            f = WO.apply_decoding_rules(logits, seq, len(init), rules)
            lsm = f - (np.max(f) + np.log(np.sum(np.exp(f[np.isfinite(f)] - np.max(f)))))
            assert abs(lps[i][k] - lsm[got[k]]) <= 0.05, (d, ops_name, i, k)
            seq.append(got[k])


@pytest.mark.parametrize("name", ["fp16-resid16", "bf16"])
def test_24_head_encoder_and_decoder_end_to_end(engine, name):
    """d = 1536 (24 heads): the encoder on the persistent GEMM (fc1 at N = 6 144, its widest) and the eight-float4 LayerNorms, the teacher-forced
    decoder and greedy decoding on the tiled kernels."""
    _encoder_decoder_end_to_end(engine, 1536, 24, name)


def test_32_head_model_on_the_tiled_kernels():
    """d = 2048 (32 heads, the decoder's limit): the encoder only runs on the tiled kernels (fc1 N = 8 192 does not fit the persistent GEMM), so in a
    context created with PCE_GEMM_FLAT=0; the default context refuses the encoder at load."""
    eng = _fresh_engine(PCE_GEMM_FLAT="0")
    try:
        _encoder_decoder_end_to_end(eng, 2048, 32, "fp16")
    finally:
        eng.close()


def test_bert_at_1536_against_the_restatement(engine, ops):
    dims = dict(BW.DIMS["mbert-base-uncased"], n_vocab=500, n_state=1536, n_head=24, n_layer=2)
    W = BW.synthetic_weights(dims, seed=13)
    rng = np.random.default_rng(3)
    toks = [rng.integers(0, dims["n_vocab"], size=n).tolist() for n in (37, 1, 64)]
    engine.bert_load(dims, BW.pack(W, dims))
    res = engine.bert_token_classify(toks)
    want = BO.forward(toks, W, dims)
    for (logits, labels), w in zip(res, want):
        assert logits.shape == w.shape
        assert np.max(np.abs(logits - w)) <= 0.08 and np.linalg.norm(logits - w) <= 3e-2 * max(np.linalg.norm(w), 1.0)


def test_loaders_refuse_the_first_width_they_cannot_run(engine):
    """PCE_E_LIMIT at load, before the blob size is looked at: the encoder at d = 1 792 (fc1 N = 7 168 past the persistent GEMM) in a default context
    and at 2 176 (34 heads, past the LayerNorms) with PCE_GEMM_FLAT=0; the decoder and BERT at 2 176."""
    blob = np.zeros(16, dtype=np.float32)
    with pytest.raises(PceError, match=r"status -5: .*persistent GEMM"):
        engine.whisper_load(dict(n_mels=80, n_ctx=1500, n_state=1792, n_head=28, n_layer=1), blob)
    with pytest.raises(PceError, match=r"status -5"):
        engine.whisper_load(dict(n_mels=80, n_ctx=1500, n_state=2048, n_head=32, n_layer=1), blob)
    with pytest.raises(PceError, match=r"status -5: .*34 heads"):
        engine.whisper_decoder_load(dict(n_vocab=64, n_text_ctx=16, n_state=34 * 64, n_head=34, n_layer=1), blob)
    with pytest.raises(PceError, match=r"status -5: .*LayerNorm"):
        engine.bert_load(dict(BW.DIMS["mbert-base-uncased"], n_state=2176, n_head=34), blob)
    eng = _fresh_engine(PCE_GEMM_FLAT="0")
    try:
        with pytest.raises(PceError, match=r"status -5: .*LayerNorm"):
            eng.whisper_load(dict(n_mels=80, n_ctx=1500, n_state=2176, n_head=34, n_layer=1), blob)
        with pytest.raises(PceError, match=r"status -1"):                   # 1 792 is a width the tiled path computes: only the blob is wrong
            eng.whisper_load(dict(n_mels=80, n_ctx=1500, n_state=1792, n_head=28, n_layer=1), blob)
    finally:
        eng.close()
