"""tests/xattn_restatement.py on the CPU: the float64 chain is the attention formula, the leaf rule is the kernel's, and the stage bounds are neither
too tight for the kernels' arithmetic nor so wide that a defect fits (tests/test_gpu_xattn.py applies the same bounds to the device's outputs).

Non-vacuity.  X.emulate restates the three kernels in float32 numpy with the operand type's roundings where the kernels have them, hi + lo included, and
takes a defect on request.  With EPS_EXP2 = 4 x 5.84e-8, over every operand class (Gaussian at every listed length, 1500 / 1499 frames, peaked, rising,
falling, the query read-out, the cancelling bv) at d = 128, 768 and 1280, leaves and pair nodes, the faithful emulation's worst |got - want| / bound is

    stage            fp16     bf16
    qp               0.550    0.729       (the 16-bit step q may have moved by is most of the bound)
    m                0.021    0.023
    l                0.010    0.010       (a worst-case score error against a random walk)
    U                0.035    0.020
    out              0.943    0.956       (one rounding of a 16-bit output: the ratio reaches 1 by construction)
    q_split          1.000    0.355       (fp16: a lo part below 2^-14 is off by exactly half its subnormal step at a tie)
    q                0.920    0.943       (one rounding of the 16-bit q)
    qp_from_bits     0.078    0.341

and every defect leaves its stage's bound on a listed case (worst ratio of that stage at d = 128 / 768 / 1280; test_every_defect_leaves_its_stage_bound
asserts > 1 where the table says caught):

    defect                            stage     fp16                     bf16                  where
    lo of Q' dropped                  q_split   1397 / 1461 / 1461       165 / 165 / 165       the read-out (Wk = I): caught at every width
    lo of P dropped                   U         1.66 / 0.15 / 0.13       12.9 / 1.25 / 1.19    Gaussian; fp16: caught at d = 128 only
    lo of U dropped                   out       12.9 / 1.75 / 0.96       29.4 / 6.96 / 5.60    cancelling bv (d = 128), Gaussian; fp16: not at 1280
    leaves cut by nt_all // 4         l, U      > 1e12                   > 1e12                every length whose tile count is no multiple of 4
    edge mask off by one frame        l, U      > 1e12                   > 1e12                every length that is no multiple of 16 (+-60000 is read)
    flat merge instead of the tree    any       0.94 / 0.70 / 0.59       0.96 / 0.89 / 0.85    NOT caught by a bound (below)

What the bounds cannot see, with the numbers:
  * P's lo at the wide widths in fp16.  The score error is taken at its worst case, (2 d / WV + WV) U sum |Q' E|, which grows with d, while P's dropped lo is
    2^-12 of a weight at every width: U's worst ratio with P rounded once to fp16 is 1.66 at d = 128 but 0.15 at d = 768 and 0.13 at d = 1280.  The margin
    on EPS_EXP2 is not what hides it: with EPS_EXP2 = 0 the three figures are 1.66, 0.15, 0.13.  In bf16 (2^-9 of a weight) it is caught at every width.
  * U's lo at d = 1280 in fp16.  It is 2^-12 of U spread over d terms, against the output's own 16-bit rounding (2^-11 of it) and the accumulation term
    (d / 2 + 4) U sum |Wv U|, which the cancelling bv leaves standing: 12.6 (cancelling bv) and 7.7 (Gaussian) at d = 128, 1.43 and 1.75 at d = 768, 0.75
    and 0.96 at d = 1280.  The cancellation case is the sharper one at d = 128 only.
  * a flat merge of the four leaves.  It is the same sum in another order: the values differ by fp32 roundings, which every bound must allow.  What pins
    the tree is bit equality on the device: the pair nodes a workgroup merges in registers (1 / 2 workgroups per clip, d <= 768) and the tree k_uv_absorb
    builds from four stored leaves (4 per clip) must give the same output bits (tests/test_gpu_xattn.py, every case)."""
import numpy as np
import pytest

from tests import xattn_restatement as X

FMTS = ("fp16", "bf16")
WORST = {}


def _note(fmt, rat, what):
    for k, r in rat.items():
        WORST[(k, fmt)] = max(WORST.get((k, fmt), 0.0), r)
    print("xattn-host", fmt, what, {k: round(float(r), 4) for k, r in rat.items()})


def test_leaf_tiles_for_every_listed_length():
    sizes = {1: (1, 0, 0, 0), 15: (1, 0, 0, 0), 16: (1, 0, 0, 0), 17: (1, 1, 0, 0), 32: (1, 1, 0, 0), 33: (1, 1, 1, 0), 48: (1, 1, 1, 0), 49: (1, 1, 1, 1),
             64: (1, 1, 1, 1), 65: (2, 2, 1, 0), 80: (2, 2, 1, 0), 81: (2, 2, 2, 0), 97: (2, 2, 2, 1), 129: (3, 3, 3, 0), 144: (3, 3, 3, 0),
             145: (3, 3, 3, 1), 160: (3, 3, 3, 1), 1499: (24, 24, 24, 22), 1500: (24, 24, 24, 22)}
    assert set(X.K_LENS) | {1499, 1500} == set(sizes) and set(X.SUBSET) <= set(X.K_LENS)
    assert [-(-k // 16) for k in X.K_LENS] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 9, 9, 10, 10]
    for k, want in sizes.items():
        lt = X.leaf_tiles(k)
        assert tuple(b - a for a, b in lt) == want, (k, lt)
        assert lt[0][0] == 0 and all(a[1] == b[0] or b[1] == b[0] for a, b in zip(lt, lt[1:])) and max(b for _, b in lt) == -(-k // 16)
        frames = [f for f0, f1, _ in X.node_frames(k, 4) for f in range(f0, f1)]
        assert frames == list(range(k)) == [f for f0, f1, _ in X.node_frames(k, 2) for f in range(f0, f1)]
    # the subset has one length per leaf pattern of the full list
    pattern = lambda k: tuple(b - a for a, b in X.leaf_tiles(k))
    assert {pattern(k) for k in X.SUBSET} == {pattern(k) for k in X.K_LENS}


@pytest.mark.parametrize("d", X.WIDTHS)
def test_the_three_stages_compose_to_plain_attention(d):
    """softmax(q K^T / 8) V with K = E Wk^T, V = E Wv^T + bv, to 1e-12 of the output's scale per clip (two float64 sums in different orders), through the
    leaves and through the pair nodes"""
    lens = (X.K_LENS if d in X.FULL_WIDTHS else X.SUBSET) + ((1500, 1499) if d == 128 else ())
    for fmt in FMTS:
        case = X.gaussian_case(d, lens, fmt, seed=1)
        want = X.plain(case, fmt)
        for nodes in (4, 2):
            got = X.composed(case, fmt, nodes)
            rel = np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)
            assert rel.max() <= 1e-12, (d, fmt, nodes, float(rel.max()))


def _classes(d, fmt):
    """every operand class of tests/test_gpu_xattn.py at width d, shaped along the EMULATION's Q' -> [(name, case)]"""
    qp_of = lambda case: (lambda g: (g["qp_hi"] + g["qp_lo"])[:, :case["heads"]])(X.emulate(case, fmt))
    out = [("gaussian", X.gaussian_case(d, X.K_LENS, fmt, seed=1))]
    pk = X.gaussian_case(d, X.PEAK_LENS, fmt, seed=3)
    out.append(("peak", X.shaped_scores(pk, qp_of(pk), "peak", fmt, X.PEAK_AT)))
    mono = X.gaussian_case(d, X.MONOTONE_LENS, fmt, seed=4)
    out += [(p, X.shaped_scores(mono, qp_of(mono), p, fmt)) for p in ("rising", "falling")]
    out.append(("cancel", X.cancelling_case(X.gaussian_case(d, [160, 97, 17], fmt, seed=6), fmt)))
    if d == 128:
        out.append(("1500", X.gaussian_case(d, [1500, 1499], fmt, seed=2)))
    return out


_CACHE = {}


def _ratios(d, fmt, defect, names=None, node_kinds=(4, 2)):
    """{(class, nodes): stage ratios} of the emulation with the defect over the classes named (default: all), the read-out included (class "readout")"""
    key = (d, fmt, defect, names, node_kinds)
    if key not in _CACHE:
        if (d, fmt) not in _CACHE:
            _CACHE[(d, fmt)] = [(name, case, X.stage1(case, fmt)) for name, case in _classes(d, fmt)]
        with np.errstate(all="ignore"):
            res = {}
            for name, case, s1 in _CACHE[(d, fmt)]:
                if names is None or name in names:
                    for nodes in node_kinds:
                        res[(name, nodes)] = X.stage_ratios(case, X.emulate(case, fmt, nodes, defect), fmt, s1=s1)
            if names is None or "readout" in names:
                rd = X.gaussian_case(d, [16] * 17, fmt, seed=5)
                res[("readout", 4)] = X.readout_ratios(rd, X.emulate(X.readout_case(rd), fmt, 4, defect), X.emulate(rd, fmt, 4, defect), fmt)
        _CACHE[key] = res
    return _CACHE[key]


def _worst(res, stages, classes=None):
    return max(r[s] for (name, _), r in res.items() for s in stages if s in r and (classes is None or name in classes))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("d", [128, 768, 1280])
def test_the_kernels_arithmetic_stays_inside_every_stage_bound(d, fmt):
    for (name, nodes), rat in _ratios(d, fmt, None).items():
        _note(fmt, rat, (d, name, nodes))
        assert all(r <= 1.0 for r in rat.values()), (d, fmt, name, nodes, rat)
    print("xattn-host worst so far", {k: round(v, 4) for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("fmt", FMTS)
def test_every_defect_leaves_its_stage_bound(fmt):
    # every class at d = 128; at the wide ones what each defect needs: the read-out for Q', Gaussian leaves and the cancelling bv for the rest
    need = dict(q_lo=("readout",), p_lo=("gaussian", "readout"), u_lo=("gaussian", "cancel"), flat_merge=("gaussian", "cancel"), leaf_floor=("gaussian",),
                mask_off_by_one=("gaussian",))
    at = {d: {df: _ratios(d, fmt, df) if d == 128 else _ratios(d, fmt, df, need[df], (4,)) for df in X.DEFECTS} for d in (128, 768, 1280)}
    show = lambda df, stages, classes=None: {d: round(float(min(_worst(at[d][df], stages, classes), 1e12)), 3) for d in at}
    print("xattn-host defects", fmt, {df: show(df, st) for df, st in (("q_lo", ("q_split",)), ("p_lo", ("U",)), ("u_lo", ("out",)), ("flat_merge", ("out", "U", "l")),
                                                                     ("leaf_floor", ("l", "U")), ("mask_off_by_one", ("l", "U")))})
    for d in at:
        assert _worst(at[d]["q_lo"], ("q_split",), ("readout",)) > 1.0, d                  # Q' lo: at the read-out, every width
        assert _worst(at[d]["leaf_floor"], ("l", "U")) > 1.0 and _worst(at[d]["mask_off_by_one"], ("l", "U")) > 1.0, d
        # a defect of one stage does not leak into the verdict on the stage before it
        assert _worst(at[d]["p_lo"], ("qp", "q_split", "q", "qp_from_bits")) <= 1.0 and _worst(at[d]["u_lo"], ("qp", "m", "l", "U")) <= 1.0, d
        # the flat merge is the same sum in another order: no bound can tell (module docstring)
        assert _worst(at[d]["flat_merge"], ("qp", "m", "l", "U", "out")) <= 1.0, d
    assert _worst(at[128]["p_lo"], ("U",), ("gaussian", "peak")) > 1.0                     # P lo: d = 128 (fp16: only there, module docstring)
    assert _worst(at[128]["u_lo"], ("out",), ("cancel",)) > 1.0                            # U lo: the cancelling bv
    if fmt == "bf16":
        assert _worst(at[768]["p_lo"], ("U",)) > 1.0 and _worst(at[1280]["u_lo"], ("out",), ("cancel",)) > 1.0
