"""The kernels that turn a decoding step's logits into tokens -- k_decode_rules, and k_step_advance behind it in the device-resident loop -- alone, on
host arrays, through the launches pce_whisper_decode_step_ex and pce_whisper_decode_loop make (pce_selftest_decode_rules), in both operand builds
(the kernels are compiled into each).  The reference is tests/decode_rules_restatement.py, float64, pinned to oracle/whisper_oracle.py and
Aligners/decoding.py by tests/test_decode_rules_host.py.  Every row of every call is checked.

What is exact.  The filters only replace logits by -inf and the arg-max compares fp32 values, so in greedy mode the chosen id must EQUAL the
restatement's with no margin, ties included (first maximum).  The one piece of arithmetic on the way to a greedy decision is the mass rule
lse_ts > m_text; every greedy row here is asserted (an assertion on the INPUT) to sit at least MASS_K = 4 bounds of lse_ts away from that threshold,
and test_mass_rule_threshold builds rows at exactly +-4 bounds.  All integer outputs of the loop form are exact, and its log-probabilities
equal, bit for bit, the step form's on the same prefix.

Bounds, U = 2^-24, derived from the kernel's fp32 chain, not fitted.  Every log-sum-exp of the kernel is  m + log(tot),  tot = sum_v exp(x_v - m):
  * d_v = x_v - m is one fp32 subtraction: the exponential's argument moves by U |d_v|, its value by the factor e^(U |d_v|);
  * the exponential is within EPS_EXP relative (tests/test_gpu_attention.py's figure for the same fp32 instruction);
  * a term's path to tot: 51 sequential additions in its thread (DR_K slots), 6 shuffle levels, 16 additions over the waves: (1 + U)^73.
  All terms are positive, so tot is within  r = sum_v w_v (e^(U |d_v|) (1 + EPS_EXP) (1 + U)^73 - 1)  relative, w the float64 softmax weights, and
  log(tot) within -log(1 - r) plus the logarithm's own EPS_LOG |log tot|.  Terms below the smallest normal number (flushed) add at most
  n_vocab 2^-126 to a tot >= 1: TINY = 2^-100 covers them.
  - log-probability  -log(sum exp(x - x[choice])):  |got - want| <= -log(1 - r) + EPS_LOG |want| + TINY.  The sum holds the choice's own term
    e^0 = 1, so tot >= 1 also when a sampled choice is not the maximum and other terms exceed 1.
  - mass rule  lse_ts = m_ts + log(tot):  the same with one more rounding of the addition: -log(1 - r) + EPS_LOG |log tot| + U |lse_ts|.
  - probe  exp(x_p - m) / tot  over the unfiltered row:  relative e^(U |d_p|) (1 + EPS_EXP) (1 + U) / (1 - r) - 1  (the division is correctly rounded:
    the library is built without fast-math), plus 2^-120 for a quotient below the smallest normal number.
  - a perturbed value  x (1 / T) - log(-log u)  (u is exact in fp32): the reciprocal and the product round once each, 2 U |x / T|; the inner
    logarithm is within EPS_LOG relative, which moves the outer one by EPS_LOG absolutely, and the outer one adds EPS_LOG |g|, g = log(-log u);
    the subtraction rounds once, U |value|:  err = 2 U |x / T| + EPS_LOG (1 + |g|) + U |value|.  A draw is EXCUSED when some other candidate's
    value + err reaches the winner's value - err; every other draw must equal the restatement's.  At most 1 % may be excused; the top-two gap of
    Gumbel-perturbed values is about Exp(1)-distributed whatever the vocabulary, and err is below 1e-4 here, so the inputs alone stay far inside
    (tests/test_decode_rules_host.py asserts the share of these very inputs on the CPU).

EPS_LOG.  Neither the headers nor the documents installed with the compiler state an accuracy for the device's logf (__logf is __builtin_logf in
this toolchain's __clang_hip_math.h: the precise form, the library being built without fast-math).  It is therefore probed, as EPS_EXP was
(test_log_probe, printed and asserted on every run): a row of K logits 0.0 and nothing else gives tot = K exactly (e^0 = 1 and sums of ones are
exact), hence -log K from the logarithm alone, for K = 2, 3, 5, 7, 10, 100, 1000, 1024, 1025, 51865, 52224.  EPS_LOG = 4 x max(EPS_LOG_MEASURED,
2^-23): the margin covers arguments the probe does not see, and one ulp is the floor of what a rounded fp32 result can promise.
Measured on an MI355X, both builds alike: worst |got + log K| / log K = 6.608e-8 = 1.11 x 2^-24 (EPS_LOG_MEASURED), below the floor: EPS_LOG = 2^-21.

Worst |got - want| / bound seen on an MI355X with these constants (the fp16 and the bf16 build agree in every digit: the kernels hold no 16-bit operand):
    log-probability, greedy             5.46e-4        with EPS_EXP = 0 (printed, not asserted)   0.0722
    log-probability, sampled            2.81e-3
    probe                               2.00e-3        with EPS_EXP = 0 (printed, not asserted)   0.480
    ids, greedy                         all equal, none excused; mass rule decided as the restatement at +-4 bounds
    ids, sampled                        0 of 256 excused at every vocabulary and temperature, all equal
    loop form                           every integer equal; out_lp bit-identical to the step form's
The asserted bounds sit three orders above the figures because EPS_EXP is the attention probe's resolution, not the exponential's error (see
tests/test_gpu_attention.py); the tests therefore also print the ratio against the same bound with EPS_EXP = 0, and a change that moves those
figures from 0.07 / 0.5 towards 1 deserves a look even while the asserted bound holds."""
import zlib

import numpy as np
import pytest

from prosody_control_french_tts_amd import PceError
from tests import decode_rules_restatement as DR
from tests.test_gpu_attention import EPS_EXP

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -100
EPS_LOG_MEASURED = 6.608e-8             # test_log_probe on an MI355X, both builds (see the docstring)
EPS_LOG = 4 * max(EPS_LOG_MEASURED, 2.0 ** -23)
MASS_K = 4                              # greedy rows keep MASS_K bounds of lse_ts between the mass rule's two sides
PLANT = np.float32(1e30)                # in the padding columns n_vocab .. ld - 1: would win every maximum if read
SENT_I, SENT_F = -777, np.float32(-777.0)
VOCABS = (300, 1024, 1025, 51865, 51866, 52224)
T_CAP = 448


# ---------------------------------------------------------------------------------------------------------------------------------------
# vocabularies, rule states and rows
# ---------------------------------------------------------------------------------------------------------------------------------------
class Vocab:
    """text ids | end-of-text | 19 specials | timestamps, as Whisper orders them.  mask: the suppress list (some text ids, the specials but one,
    <|notimestamps|> = the last special) in bit 0, blank and end-of-text in bit 1.  only_eot: every special suppressed."""

    def __init__(self, V, only_eot=False, all_masked=False):
        self.V, self.ld = V, -(-V // 128) * 128
        self.n_ts = min(1501, V // 4)
        self.ts = V - self.n_ts
        self.eot = self.ts - 20
        m = np.zeros(V, np.uint8)
        m[self.eot + 1:self.ts] = 1
        if not only_eot:
            m[self.eot + 3] = 0                                   # one special the suppress list leaves alone
        m[[3, 11, self.eot - 1]] |= 1
        m[[5, self.eot]] |= 2
        if all_masked:
            m[:] = 1
        self.mask = m
        self.prompt = [self.eot + 1, self.eot + 7, self.eot + 9]
        self.pad = V - 1                                          # pads of the token rows: a timestamp, would move the floor if read

    def text(self, k):
        return 20 + (k * 37) % (self.eot - 40)                    # some unmasked text id

    def stamp(self, k):
        return self.ts + k


def rule_states(vc, per_clip):
    """Every rule state, as (name, tokens, sample_begin).  per_clip: prompts of three lengths (else sample_begin = 3 for all)."""
    P, t, s, e = vc.prompt, vc.text, vc.stamp, vc.eot
    top = vc.V - 1
    tails = [("ns0", []), ("ns1-text", [t(1)]), ("ns1-ts", [s(4)]),
             ("ns2-text-text", [t(1), t(2)]), ("ns2-text-ts", [t(1), s(4)]), ("ns2-ts-text", [s(4), t(2)]), ("ns2-ts-ts", [s(4), s(4)]),
             ("many-text-text", [s(0), t(1), s(2), s(2), t(3), t(4)]), ("many-text-ts", [s(0), t(1), s(2), s(2), t(3), s(6)]),
             ("many-ts-text", [s(0), t(1), s(2), s(2), s(5), t(4)]), ("many-ts-ts", [s(0), t(1), t(2), t(3), s(6), s(6)]),
             ("many-no-ts", [t(1), t(2), t(3), t(4), t(5), t(6)]),
             ("closed-pair", [s(0), t(1), s(2), s(2)]), ("closed-pair-text-ts", [s(0), t(1), s(2), s(2), t(3), s(8)]),
             ("early-ts-then-text", [s(9), t(1), t(2), t(3)]),
             ("top-stamp-pair", [t(1), top, top]), ("top-stamp-open", [t(1), top]), ("top-stamp-then-text", [top, top, t(2)]),
             ("ended", [s(0), t(1), s(3), e]), ("ended-at-once", [e]), ("ended-long-ago", [t(1), e, e, e])]
    out = []
    for j, (name, tail) in enumerate(tails):
        prompt = list(P)
        if per_clip:
            prompt = [P[0]] * (j % 3) + prompt                    # lengths 3, 4, 5
        out.append((name, prompt + tail, len(prompt)))
    # timestamps in the prompt, before sample_begin: ignored (previous-text prompts hold none in practice; the rule says `sampled tokens`)
    pp = [s(30), s(31), P[0]]
    out += [("prompt-ts-ns0", pp, 3), ("prompt-ts-ns1", pp + [t(1)], 3), ("prompt-ts-ns2", pp + [t(1), s(2)], 3),
            ("prompt-ends-eot", P[:2] + [e], 3)]
    return out


def noise_rows(vc, names, seed, sigma=3.0):
    """one float32 row [V] per state name, drawn from (seed, name): a state keeps its row in whatever batch it sits"""
    rows = []
    for name in names:
        rows.append((np.random.default_rng([seed, vc.V, zlib.crc32(name.encode())]).standard_normal(vc.V) * sigma).astype(np.float32))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------------
# bounds (see the module docstring)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tot_rel(d, eps_exp):
    """relative bound of tot = sum exp(d) as the kernel adds it (d: float64, finite entries only)"""
    d = d[np.isfinite(d)]
    w = np.exp(d - d.max())
    w /= w.sum()
    return float((w * (np.exp(U * np.abs(d)) * (1 + eps_exp) * (1 + U) ** 73 - 1)).sum())


def lp_bound(xf, choice, eps_exp=EPS_EXP):
    d = xf[np.isfinite(xf)] - xf[choice]
    want = -np.log(np.exp(d - d.max()).sum()) - d.max()
    return -np.log1p(-_tot_rel(d, eps_exp)) + EPS_LOG * abs(want) + TINY


def mass_bound(xf_before_mass, ts, eps_exp=EPS_EXP):
    """bound of lse_ts over the timestamps of a row filtered up to (not including) the mass rule; 0 without a finite timestamp"""
    x = xf_before_mass[ts:]
    x = x[np.isfinite(x)]
    if not x.size:
        return 0.0
    d = x - x.max()
    log_tot = float(np.log(np.exp(d).sum()))
    return -np.log1p(-_tot_rel(d, eps_exp)) + EPS_LOG * abs(log_tot) + U * abs(x.max() + log_tot)


def probe_bound(row, token, eps_exp=EPS_EXP):
    x = np.asarray(row, np.float64)
    d = x - x.max()
    want = np.exp(d[token]) / np.exp(d).sum()
    rel = np.exp(U * abs(d[token])) * (1 + eps_exp) * (1 + U) / (1 - _tot_rel(d, eps_exp)) - 1
    return want * rel + 2.0 ** -120


def perturbed_err(xf, p, g, temperature):
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(xf), 2 * U * np.abs(xf / temperature) + EPS_LOG * (1 + np.abs(g)) + U * np.abs(p), 0.0)


def draw_margin(xf, p, g, temperature):
    """(winner's value - err) - max over the others of (value + err): a draw with a margin <= 0 is excused"""
    e = perturbed_err(xf, p, g, temperature)
    i = int(np.argmax(p))
    hi = np.where(np.isfinite(p), p + e, -np.inf)
    hi[i] = -np.inf
    return float(p[i] - e[i] - hi.max())


RATIOS = {}


def _ratio(check, build, what, diff, bound, asserted=True):
    diff, bound = np.atleast_1d(diff), np.atleast_1d(bound)
    r = float(np.max(diff / bound)) if diff.size else 0.0
    key = (check, build)
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    print(f"decode-ratio {check} {build} {what}: {r:.3e} (worst so far {RATIOS[key]:.3e})")
    assert not asserted or not (diff > bound).any(), (check, build, what, r, np.argwhere(diff > bound)[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------------
# running the hook, and what the restatement expects of a call
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=["fp16", "bf16"])
def eng(request, engine):
    """the engine on one operand build (k_decode_rules and k_step_advance are compiled into each)"""
    engine.whisper_set_operands(request.param)
    engine.build_name = request.param
    return engine


def padded(vc, rows):
    """[1][n][ld] float32: the rows, +1e30 in the padding columns"""
    x = np.full((1, len(rows), vc.ld), PLANT, np.float32)
    for i, r in enumerate(rows):
        x[0, i, :vc.V] = r
    return x


def run_step(eng, vc, rows, seqs, sb, form=0, max_initial=None, temperature=0.0, seed=0, probe_token=-1, keys=None, extra=3, t_cap=T_CAP):
    """One step over the rows -> (next, log-probability, probe) [n], through the step form or one step of the loop form (whose probe stays as it went
    in).  The outputs go in `extra` elements longer, filled with sentinels, and the call must leave those alone."""
    n = len(rows)
    logits = padded(vc, rows)
    kw = dict(max_initial_timestamp_index=max_initial, temperature=temperature, seed=seed, sample_keys=keys, t_cap=t_cap)
    if form == 0:
        nxt, lp, pr = np.full(n + extra, SENT_I, np.int32), np.full(n + extra, SENT_F), np.full(n + extra, SENT_F)
        eng.selftest_decode_rules(0, vc.V, logits, seqs, sb, vc.eot, vc.ts, vc.mask, nxt, lp, pr, probe_token=probe_token, pad_token=vc.pad, **kw)
        assert np.all(nxt[n:] == SENT_I) and np.all(lp[n:] == SENT_F) and np.all(pr[n:] == SENT_F)
        return nxt[:n], lp[:n], pr[:n]
    out_tok, out_lp = np.full(n + extra, SENT_I, np.int32), np.full(n + extra, SENT_F)
    table = np.full((n, t_cap), vc.pad, np.int32)
    state = np.full(10 * n + 2 + extra, SENT_I, np.int32)
    eng.selftest_decode_rules(1, vc.V, logits, seqs, sb, vc.eot, vc.ts, vc.mask, out_tok, out_lp, max_new=1, table=table, loop_state=state, **kw)
    assert np.all(out_tok[n:] == SENT_I) and np.all(out_lp[n:] == SENT_F) and np.all(state[10 * n + 2:] == SENT_I)
    return out_tok[:n], out_lp[:n], None


_WANT = {}


def want_greedy(vc, rows, seqs, sbs, max_initial, tag, exact_mass=False):
    """per row: (id, log-probability, bound, bound at EPS_EXP = 0), asserting the INPUT keeps its distance from the mass rule's threshold (the rule
    only touches text ids, so the filtered row still holds the timestamps it summed); cached per tag (both builds ask for the same rows).
    exact_mass: rows whose timestamp mass is computed without any rounding (see test_ties) may sit ON the threshold."""
    if tag in _WANT:
        return _WANT[tag]
    out = []
    for row, seq, sb in zip(rows, seqs, sbs):
        xf, margin = DR.filtered(row, seq, sb, vc.eot, vc.ts, vc.mask, max_initial)
        if np.isfinite(margin) and not (exact_mass and margin == 0.0):
            assert abs(margin) > MASS_K * mass_bound(xf, vc.ts), ("input too close to the mass rule's threshold", tag, margin)
        i, lp = DR.choose(xf, seq, vc.eot)
        live = np.isfinite(xf.max()) and not (seq and seq[-1] == vc.eot)
        out.append((i, lp, lp_bound(xf, i) if live else 0.0, lp_bound(xf, i, 0.0) if live else 0.0))
    _WANT[tag] = out
    return out


def check_greedy(eng, vc, rows, seqs, sb, form, max_initial, tag, probe_token=-1, exact_mass=False):
    sbs = [sb] * len(rows) if np.isscalar(sb) else list(sb)
    want = want_greedy(vc, rows, seqs, sbs, max_initial, tag, exact_mass)
    nxt, lp, pr = run_step(eng, vc, rows, seqs, sb, form, max_initial, probe_token=probe_token)
    assert nxt.tolist() == [w[0] for w in want], (tag, form, [(k, int(a), w[0]) for k, (a, w) in enumerate(zip(nxt, want)) if a != w[0]][:6])
    exact = np.array([w[2] == 0.0 for w in want])
    assert np.all(lp[exact] == 0.0), tag                            # ended sequences and rows without a candidate: exactly 0
    if (~exact).any():
        diff = np.abs(lp.astype(np.float64) - np.array([w[1] for w in want]))[~exact]
        _ratio("logprob", eng.build_name, tag, diff, np.array([w[2] for w in want])[~exact])
        _ratio("logprob, EPS_EXP = 0 (printed only)", eng.build_name, tag, diff, np.array([w[3] for w in want])[~exact], asserted=False)
    if probe_token >= 0 and form == 0:
        wp = np.array([DR.probe(r, probe_token) for r in rows])
        _ratio("probe", eng.build_name, tag, np.abs(pr.astype(np.float64) - wp), np.array([probe_bound(r, probe_token) for r in rows]))
        _ratio("probe, EPS_EXP = 0 (printed only)", eng.build_name, tag, np.abs(pr.astype(np.float64) - wp),
               np.array([probe_bound(r, probe_token, 0.0) for r in rows]), asserted=False)
    return nxt, lp, pr


# ---------------------------------------------------------------------------------------------------------------------------------------
# the logarithm's probe
# ---------------------------------------------------------------------------------------------------------------------------------------
LOG_KS = (2, 3, 5, 7, 10, 100, 1000, 1024, 1025, 51865, 52224)


def probe_log_error(eng):
    """The measurement behind EPS_LOG (see the module docstring) -> worst |got + log K| / log K over LOG_KS"""
    V = 52224
    rows = []
    for K in LOG_KS:
        r = np.full(V, -np.inf, np.float32)
        r[:K] = 0.0
        rows.append(r)
    x = np.full((1, len(rows), V), 0, np.float32)
    x[0] = rows
    nxt, lp, pr = np.zeros(len(rows), np.int32), np.zeros(len(rows), np.float32), np.zeros(len(rows), np.float32)
    # (no timestamps: timestamp_begin = n_vocab; one sampled token so far, nothing masked)
    eng.selftest_decode_rules(0, V, x, [[V - 3, 1]] * len(rows), 1, V - 2, V, np.zeros(V, np.uint8), nxt, lp, pr)
    assert np.all(nxt == 0)
    want = -np.log(np.array(LOG_KS, np.float64))
    return float(np.max(np.abs(lp.astype(np.float64) - want) / np.abs(want)))


def test_log_probe(eng):
    got = probe_log_error(eng)
    print(f"decode-ratio log-probe {eng.build_name}: worst relative error of -log K {got:.3e} = {got / 2.0 ** -24:.2f} x 2^-24 (EPS_LOG {EPS_LOG:.3e})")
    assert got <= EPS_LOG


# ---------------------------------------------------------------------------------------------------------------------------------------
# rule states, vocabularies, magnitudes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VOCABS)
def test_rule_states(eng, V):
    """Every rule state at every vocabulary: step form and loop pitch, scalar and per-clip sample_begin, the four max_initial_timestamp_index
    settings; +1e30 in the padding columns and timestamp ids past every sequence's length.  Ids exact, log-probability and probe within bounds."""
    for only_eot in (False, True):                                 # (with every special suppressed, text + open timestamp leaves end-of-text alone below timestamp_begin)
        vc = Vocab(V, only_eot=only_eot)
        for per_clip in (False, True):
            states = rule_states(vc, per_clip)
            names, seqs, sbs = [s[0] for s in states], [s[1] for s in states], [s[2] for s in states]
            rows = noise_rows(vc, names, 1)
            rows[1][(vc.mask & 1) == 0] = -np.inf                  # one row (ns1-text) whose every candidate is masked: finite logits at suppressed ids only
            sb = sbs if per_clip else 3
            for mi in (None, 0, 50, V + 100):
                for form in (0, 1):
                    check_greedy(eng, vc, rows, seqs, sb, form, mi, ("states", V, only_eot, per_clip, mi), probe_token=vc.eot + 2 if form == 0 else -1)


@pytest.mark.parametrize("V", (300, 51865))
def test_only_end_of_text_left_and_all_masked(eng, V):
    """After text + timestamp the rules leave end-of-text and the timestamps from the floor on; with every special suppressed, end-of-text is the one id
    below timestamp_begin.  And a mask that suppresses everything: id 0, log-probability 0."""
    vc = Vocab(V, only_eot=True)
    seqs = [vc.prompt + [vc.text(1), vc.stamp(7)], vc.prompt + [vc.stamp(0), vc.text(1), vc.text(2), vc.stamp(7)]]
    rows = noise_rows(vc, ["only-eot-a", "only-eot-b"], 2)
    rows[0][vc.eot] = 40.0                                         # end-of-text wins over the timestamps' mass
    rows[1][vc.ts:] = -np.inf                                      # no timestamp left either: end-of-text is the only candidate
    for form in (0, 1):
        nxt, lp, _ = check_greedy(eng, vc, rows, seqs, 3, form, None, ("only-eot", V))
        assert nxt.tolist() == [vc.eot, vc.eot] and lp[1] == 0.0
    va = Vocab(V, all_masked=True)
    states = rule_states(va, False)
    rows = noise_rows(va, [s[0] for s in states], 3)
    for form in (0, 1):
        nxt, lp, _ = check_greedy(eng, va, rows, [s[1] for s in states], 3, form, None, ("all-masked", V))
        assert all(int(a) in (0, va.eot) for a in nxt) and np.all(lp == 0.0)


@pytest.mark.parametrize("V", (300, 51866))
def test_magnitudes(eng, V):
    """logits of +-80 and rows shifted by +1e4: without the subtraction of the maximum these overflow"""
    vc = Vocab(V)
    states = [s for s in rule_states(vc, False) if s[0] in ("ns0", "ns1-text", "ns2-text-ts", "many-ts-ts", "many-text-text", "early-ts-then-text")]
    names, seqs = [s[0] for s in states], [s[1] for s in states]
    base = noise_rows(vc, names, 4, sigma=1.0)
    wide = [(r * (80.0 / np.abs(r).max())).astype(np.float32) for r in base]
    shifted = [(r * 3.0 + np.float32(1e4)).astype(np.float32) for r in base]
    for kind, rows in (("pm80", wide), ("plus1e4", shifted)):
        for form in (0, 1):
            check_greedy(eng, vc, rows, seqs, 3, form, None, ("magnitudes", kind, V), probe_token=7 if form == 0 else -1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the mass rule at its threshold, ties
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (300, 51865))
def test_mass_rule_threshold(eng, V):
    """100 timestamps at 0 (or at 1e4) against a best text logit of log 100 -+ delta, delta = MASS_K bounds of lse_ts: below, the timestamps' mass
    exceeds every text token and the first timestamp is chosen; above, the text token.  Plus rows far from the threshold."""
    vc = Vocab(V)
    seq = vc.prompt + [vc.text(1), vc.text(2)]
    rows, want_ids = [], []
    n_ts = min(100, vc.n_ts)
    for shift in (0.0, 1e4):
        ts_val = np.float32(shift)
        probe_row = np.full(V, -np.inf, np.float64)
        probe_row[vc.ts:vc.ts + n_ts] = ts_val
        bound = mass_bound(probe_row, vc.ts)
        lse = float(ts_val) + np.log(n_ts)
        for k in (-MASS_K, MASS_K, -1000, 1000):
            txt = np.float32(lse + k * bound)
            # the text value is rounded to fp32: step outwards until the rounded value keeps MASS_K bounds
            while abs(float(txt) - lse) < MASS_K * bound:
                txt = np.nextafter(txt, np.float32(np.inf if k > 0 else -np.inf))
            r = np.full(V, np.float32(shift - 50.0), np.float32)
            r[vc.ts:] = -np.inf
            r[vc.ts:vc.ts + n_ts] = ts_val
            r[vc.text(9)] = txt
            rows.append(r)
            want_ids.append(vc.ts if k < 0 else vc.text(9))
    for form in (0, 1):
        nxt, _, _ = check_greedy(eng, vc, rows, [seq] * len(rows), 3, form, None, ("mass", V))
        assert nxt.tolist() == want_ids


@pytest.mark.parametrize("V", (1025, 51865, 51866, 52224))
def test_ties(eng, V):
    """Bit-equal maxima across the slots of one thread (ids t and t + 1024), lanes, waves and the text / timestamp boundary, also with the lower id
    masked: the lowest surviving id wins.  A lone timestamp at the text maximum sits ON the mass rule's threshold, and exactly so on the device too:
    its sum is the one term e^0 = 1 and zeros, log 1 = 0, m_ts + 0 = m_ts -- no rounding anywhere, the mass does not EXCEED the text maximum."""
    vc = Vocab(V)
    seq = vc.prompt + [vc.text(1), vc.text(2)]                     # text after text: every unmasked id may follow
    t, top = vc.ts, np.float32(7.25)
    assert vc.mask[3] & 1 and vc.mask[11] & 1
    if V == 1025:                                                  # (two slots: id 1024 is a timestamp in the second)
        groups = [[200, 201], [20, 63], [300, 300 + 64], [100, 100 + 64 * 9], [3, 3 + 64], [11, 12], [3, 11, 3 + 64, 11 + 128], [500, t + 5], [t - 21, t],
                  [t + 1, t + 2], [t + 3, t + 3 + 64], [100, 1024], [t, 1024]]
    else:
        groups = [[100, 100 + 1024], [100 + 1024 * 7, 100 + 1024 * 49], [200, 201], [20, 63], [300, 300 + 64], [1000, 1000 + 64 * 15],
                  [64 * 9 + 5, 1024 * 3 + 64 * 2 + 5, 1024 * 30 + 5], [3, 3 + 1024], [11, 12], [3, 11, 3 + 64, 11 + 1024 * 20],
                  [40000, t + 5], [t - 21, t], [t + 5, t + 5 + 1024], [t + 1, t + 2], [50 * 1024 + 7, 50 * 1024 + 71], [V - 1, V - 1 - 1024]]
    assert all(v < V for g in groups for v in g)
    rows, want_ids = [], []
    for g in groups:
        r = np.minimum(noise_rows(vc, [f"tie{g[0]}"], 5, sigma=1.0)[0], np.float32(5.0))
        r[t:] -= np.float32(20.0)                                  # (1501 timestamps of noise would outweigh the text maximum)
        if any(v >= t for v in g):
            r[t:] = -np.inf                                        # a lone timestamp: its mass EQUALS the text maximum, which does not exceed it
            if all(v >= t for v in g):
                r[:t] = np.minimum(r[:t], np.float32(-30.0))       # (timestamps only: their mass wins)
        r[g] = top
        rows.append(r)
        want_ids.append(min(v for v in g if not vc.mask[v] & 1))
    for form in (0, 1):
        nxt, _, _ = check_greedy(eng, vc, rows, [seq] * len(rows), 3, form, None, ("ties", V), exact_mass=True)
        assert nxt.tolist() == want_ids


# ---------------------------------------------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------------------------------------------
SAMPLE_ROWS, SAMPLE_SEEDS, TEMPS = 64, (11, 2 ** 40 + 6, 99, 8), (0.2, 1.0, 5.0)


def sampling_inputs(V):
    """64 rows over the rule states at lengths (positions) of their own, keys that are no batch positions"""
    vc = Vocab(V)
    states = rule_states(vc, True)
    live = [s for s in states if not s[0].startswith("ended") and s[0] != "prompt-ends-eot"]
    pick = [live[i % len(live)] for i in range(SAMPLE_ROWS)]
    seqs = [[vc.prompt[0]] * (i // len(live)) + s[1] for i, s in enumerate(pick)]
    sbs = [s[2] + i // len(live) for i, s in enumerate(pick)]
    rows = noise_rows(vc, [f"{s[0]}#{i}" for i, s in enumerate(pick)], 6)
    keys = [(i * 2654435761 + 12345) % (1 << 31) - (1 << 30) for i in range(SAMPLE_ROWS)]
    return vc, rows, seqs, sbs, keys


_SAMPLE_WANT = {}


def sampling_want(V, temperature, seed):
    """per row: (id, log-probability, log-probability bound, draw margin, x[choice] - max x), cached"""
    k = (V, temperature, seed)
    if k not in _SAMPLE_WANT:
        vc, rows, seqs, sbs, keys = sampling_inputs(V)
        out = []
        for row, seq, sb, key in zip(rows, seqs, sbs, keys):
            xf, _ = DR.filtered(row, seq, sb, vc.eot, vc.ts, vc.mask, None)
            i, lp, gap, p, g = DR.sample(xf, seq, vc.eot, temperature, seed, key)
            out.append((i, lp, lp_bound(xf, i), draw_margin(xf, p, g, temperature), float(xf[i] - xf.max())))
        _SAMPLE_WANT[k] = out
    return _SAMPLE_WANT[k]


@pytest.mark.parametrize("temperature", TEMPS)
@pytest.mark.parametrize("V", VOCABS)
def test_sampling_draws(eng, V, temperature):
    """256 (seed, key, position) triples per vocabulary and temperature: the drawn id equals the restatement's unless excused (at most 1 %), and the
    reported log-probability is the filtered, UNSCALED log-softmax at the drawn id -- also for draws far below the maximum."""
    vc, rows, seqs, sbs, keys = sampling_inputs(V)
    n_excused, n_all, deepest = 0, 0, 0.0
    for seed in SAMPLE_SEEDS:
        want = sampling_want(V, temperature, seed)
        nxt, lp, _ = run_step(eng, vc, rows, seqs, sbs, form=seed % 2, temperature=temperature, seed=seed, keys=keys)
        for k, (a, b, w) in enumerate(zip(nxt, lp, want)):
            n_all += 1
            if w[3] <= 0.0:
                n_excused += 1
                continue
            assert int(a) == w[0], (V, temperature, seed, k, int(a), w)
            deepest = min(deepest, w[4])
        ok = np.array([w[3] > 0.0 for w in want])
        _ratio("sampled logprob", eng.build_name, (V, temperature, seed), np.abs(lp.astype(np.float64) - np.array([w[1] for w in want]))[ok],
               np.array([w[2] for w in want])[ok])
    print(f"decode-ratio sampling {eng.build_name} V={V} T={temperature}: {n_excused} of {n_all} draws excused; deepest choice {deepest:.2f} below the maximum")
    assert n_excused <= 0.01 * n_all
    if temperature == 5.0:
        assert deepest < -5.0                                     # (a property of the inputs: some draws sit well below the maximum)


def test_sampling_never_draws_a_masked_id_and_covers_the_allowed(eng):
    """temperature 1e6 flattens the distribution over what the filters leave: no masked id in 64 rows x 4 seeds; and with 8 ids allowed, 400 seeds draw
    every one of them (each draw equal to the restatement's)."""
    vc, rows, seqs, sbs, keys = sampling_inputs(300)
    for seed in SAMPLE_SEEDS:
        nxt, lp, _ = run_step(eng, vc, rows, seqs, sbs, temperature=1e6, seed=seed, keys=keys)
        for a, row, seq, sb in zip(nxt, rows, seqs, sbs):
            xf, _ = DR.filtered(row, seq, sb, vc.eot, vc.ts, vc.mask, None)
            assert np.isfinite(xf[int(a)]), (seed, int(a))
    allowed = [20, 21, 64, 100, 150, 199, vc.eot, vc.eot + 3]
    row = np.full(vc.V, -np.inf, np.float32)
    row[allowed] = np.linspace(-1.0, 1.0, 8, dtype=np.float32)
    seq = vc.prompt + [vc.text(1), vc.text(2)]
    xf, _ = DR.filtered(row, seq, 3, vc.eot, vc.ts, vc.mask, None)
    seen = set()
    for seed in range(400):
        nxt, lp, _ = run_step(eng, vc, [row], [seq], 3, temperature=1.0, seed=seed, extra=0)
        i, wlp, gap, p, g = DR.sample(xf, seq, vc.eot, 1.0, seed, 0)
        assert draw_margin(xf, p, g, 1.0) <= 0.0 or int(nxt[0]) == i, (seed, int(nxt[0]), i)
        seen.add(int(nxt[0]))
    assert seen == set(allowed)


def test_sampling_keys_positions_and_lengths(eng):
    """With sample_keys a row draws the same id wherever it sits and whatever it is batched with; without them the batch position is the key; and
    the sequence length alone changes the draws."""
    vc, rows, seqs, sbs, keys = sampling_inputs(1025)
    n = 16
    rows, seqs, sbs, keys = rows[:n], seqs[:n], sbs[:n], keys[:n]
    a, la, _ = run_step(eng, vc, rows, seqs, sbs, temperature=1.0, seed=3, keys=keys)
    b, lb, _ = run_step(eng, vc, rows[::-1], seqs[::-1], sbs[::-1], temperature=1.0, seed=3, keys=keys[::-1])
    assert np.array_equal(a, b[::-1]) and np.array_equal(la.view(np.int32), lb[::-1].view(np.int32))
    c, lc, _ = run_step(eng, vc, rows[5:9], seqs[5:9], sbs[5:9], temperature=1.0, seed=3, keys=keys[5:9])
    assert np.array_equal(a[5:9], c) and np.array_equal(la[5:9].view(np.int32), lc.view(np.int32))

    def want(order, key_of, extra_len=0):
        out = []
        for pos, k in enumerate(order):
            seq = [vc.prompt[0]] * extra_len + seqs[k]
            xf, _ = DR.filtered(rows[k], seq, sbs[k] + extra_len, vc.eot, vc.ts, vc.mask, None)
            i, _, _, p, g = DR.sample(xf, seq, vc.eot, 1.0, 3, key_of(pos, k))
            out.append((i, draw_margin(xf, p, g, 1.0)))
        return out
    # without keys: the batch position
    order = list(range(n))
    d, _, _ = run_step(eng, vc, rows, seqs, sbs, temperature=1.0, seed=3)
    e, _, _ = run_step(eng, vc, rows[::-1], seqs[::-1], sbs[::-1], temperature=1.0, seed=3)
    wd, we = want(order, lambda pos, k: pos), want(order[::-1], lambda pos, k: pos)
    assert all(m <= 0 or int(x) == i for x, (i, m) in zip(d, wd)) and all(m <= 0 or int(x) == i for x, (i, m) in zip(e, we))
    assert [w[0] for w in wd] != [w[0] for w in we][::-1]          # (the inputs do tell the two keyings apart)
    # one more prompt token in front: the same rule state and row, another position
    f, _, _ = run_step(eng, vc, rows, [[vc.prompt[0]] + s for s in seqs], [s + 1 for s in sbs], temperature=1.0, seed=3, keys=keys)
    wf = want(order, lambda pos, k: keys[k], extra_len=1)
    assert all(m <= 0 or int(x) == i for x, (i, m) in zip(f, wf))
    assert not np.array_equal(a, f)


# ---------------------------------------------------------------------------------------------------------------------------------------
# batch independence, sentinels
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", (0.0, 1.0))
def test_batch_independence(eng, temperature):
    """A row's three outputs are bit-identical alone, in a batch of 37 mixed states, and in the reversed batch"""
    vc = Vocab(1025)
    states = (rule_states(vc, True) + rule_states(vc, False))[:37]
    names, seqs, sbs = [f"{s[0]}@{i}" for i, s in enumerate(states)], [s[1] for s in states], [s[2] for s in states]
    rows = noise_rows(vc, names, 7)
    keys = list(range(500, 537))
    kw = dict(temperature=temperature, seed=21, probe_token=vc.eot + 2)
    bits_of = lambda r: (r[0].tolist(), r[1].view(np.int32).tolist(), r[2].view(np.int32).tolist())
    whole = bits_of(run_step(eng, vc, rows, seqs, sbs, keys=keys, **kw))
    rev = bits_of(run_step(eng, vc, rows[::-1], seqs[::-1], sbs[::-1], keys=keys[::-1], **kw))
    assert [v[::-1] for v in rev] == list(whole)
    for i in range(37):
        alone = bits_of(run_step(eng, vc, rows[i:i + 1], seqs[i:i + 1], sbs[i:i + 1], keys=keys[i:i + 1], **kw))
        assert [v[0] for v in alone] == [v[i] for v in whole], i


def test_probe_off_leaves_probe_prob_alone(eng):
    vc = Vocab(300)
    states = rule_states(vc, False)[:5]
    rows = noise_rows(vc, [s[0] for s in states], 8)
    nxt, lp, pr = run_step(eng, vc, rows, [s[1] for s in states], 3, probe_token=-1)
    assert np.all(pr == SENT_F) and np.all(nxt != SENT_I) and np.all(lp != SENT_F)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loop form
# ---------------------------------------------------------------------------------------------------------------------------------------
LOOP_STEPS, LOOP_CAP = 12, 40


def loop_script(n, seed=0):
    """Scripted logits [12][n][V = 300]: noise plus a spike at what each sequence is steered towards -- timestamp pairs, text, rising timestamps,
    end-of-text at different steps (the rules may overrule the spike; the restatement follows them).  Every third sequence from the second on starts
    so long that it reaches the table's pitch mid-run."""
    vc = Vocab(300)
    rng = np.random.default_rng([seed, n])
    prompts, sbs = [], []
    for i in range(n):
        L = 3 + i % 3
        if i % 3 == 1:
            L = LOOP_CAP - 2 - (i // 3) % 6                        # reaches LOOP_CAP after 2 .. 7 steps
        prompts.append([vc.prompt[0]] * (L - 3) + vc.prompt)
        sbs.append(L)
    logits = (rng.standard_normal((LOOP_STEPS, n, vc.V)) * 2.0).astype(np.float32)
    for i in range(n):
        stamp, stop = 0, 4 + (i * 5) % 11                          # end-of-text steered at steps 4 .. 14 (some never within 12)
        for s in range(LOOP_STEPS):
            kind = (s + i) % 4
            if s == 0:
                target = vc.stamp(0)
            elif s >= stop:
                target = vc.eot
            elif kind in (0, 1):
                target = vc.text(int(rng.integers(0, 1000)))
            else:
                stamp += int(rng.integers(0, 3)) if kind == 3 else 0
                stamp += 1 if kind == 2 else 0
                target = vc.stamp(min(stamp, vc.n_ts - 1))
            logits[s, i, target] += 30.0
    return vc, prompts, sbs, logits


def loop_want(vc, prompts, sbs, logits, max_new, steps):
    befores = []

    def choices(step, table):
        if step >= steps:
            return None
        befores.append([list(s) for s in table])
        out = []
        for i, seq in enumerate(table):
            xf, margin = DR.filtered(logits[step, i], seq, sbs[i], vc.eot, vc.ts, vc.mask, 1)
            assert not np.isfinite(margin) or abs(margin) > MASS_K * mass_bound(xf, vc.ts), ("scripted row near the mass rule's threshold", step, i, margin)
            out.append(DR.choose(xf, seq, vc.eot))
        return out
    return DR.loop(choices, prompts, LOOP_CAP, vc.eot, max_new), befores


@pytest.mark.parametrize("n,max_new", [(3, 12), (3, 20), (300, 12), (300, 20)])
def test_loop_form(eng, n, max_new):
    """12 scripted steps of k_decode_rules + k_step_advance: every integer output equals the Python restatement, out_lp equals the step form's
    log-probability of the same prefix bit for bit, and what no launch writes keeps its sentinel.  n = 300 runs the 256-thread stride loop."""
    vc, prompts, sbs, logits = loop_script(n)
    want, befores = loop_want(vc, prompts, sbs, logits, max_new, LOOP_STEPS)
    x = np.full((LOOP_STEPS, n, vc.ld), PLANT, np.float32)
    x[:, :, :vc.V] = logits
    out_tok, out_lp = np.full((n, max_new), SENT_I, np.int32), np.full((n, max_new), SENT_F)
    table = np.full((n, LOOP_CAP), vc.pad, np.int32)
    state = np.full(10 * n + max_new + 1 + 4, SENT_I, np.int32)
    eng.selftest_decode_rules(1, vc.V, x, prompts, sbs, vc.eot, vc.ts, vc.mask, out_tok, out_lp, max_initial_timestamp_index=1, t_cap=LOOP_CAP,
                              max_new=max_new, table=table, loop_state=state)
    assert out_tok[:, :LOOP_STEPS].tolist() == want["out_tok"]
    assert np.all(out_tok[:, LOOP_STEPS:] == SENT_I) and np.all(out_lp[:, LOOP_STEPS:] == SENT_F)
    ln, ended, ct = state[:n], state[n:2 * n], state[2 * n:10 * n].reshape(8, n)
    n_ended, counter, tail = state[10 * n:10 * n + max_new], state[10 * n + max_new], state[10 * n + max_new + 1:]
    assert ln.tolist() == want["len"] and ended.tolist() == want["ended"] and int(counter) == LOOP_STEPS and np.all(tail == SENT_I)
    assert n_ended.tolist() == want["n_ended"] + [0] * (max_new - LOOP_STEPS)
    assert ct[0].tolist() == want["ct_tok"] and ct[4].tolist() == want["ct_keys"] and ct[7].tolist() == want["ct_pos"]
    assert np.all(ct[[1, 2, 3, 5, 6]] == SENT_I)
    for i in range(n):
        assert table[i, :ln[i]].tolist() == want["table"][i] and np.all(table[i, ln[i]:] == vc.pad), i
    assert max(want["len"]) == LOOP_CAP and 0 < sum(want["ended"]) and want["n_ended"][0] == 0          # (the script reaches what it is meant to)
    # the same prefixes through the step form: bit-identical log-probabilities, the same ids
    for s in range(LOOP_STEPS):
        nxt, lp, _ = run_step(eng, vc, list(logits[s]), befores[s], sbs, form=0, max_initial=1, extra=0, t_cap=LOOP_CAP)
        assert nxt.tolist() == out_tok[:, s].tolist(), s
        assert np.array_equal(lp.view(np.int32), out_lp[:, s].view(np.int32)), s


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(eng):
    """Everything the hook refuses, before anything is launched: the outputs keep their sentinels"""
    vc = Vocab(300)
    seqs = [vc.prompt + [vc.text(1)], vc.prompt]
    good = dict(form=0, V=300, eot=vc.eot, ts=vc.ts, seqs=seqs, sb=3, mask=vc.mask, ld=vc.ld, steps=1, n_out=2, t_cap=T_CAP, max_new=0, kw={})

    def refused(**over):
        a = dict(good, **over)
        n = len(a["seqs"])
        logits = np.zeros((a["steps"], n, a["ld"]), np.float32)
        out_tok, out_lp, pr = np.full(a["n_out"], SENT_I, np.int32), np.full(a["n_out"], SENT_F), np.full(a["n_out"], SENT_F)
        table = np.full(a.get("table_elems", n * a["t_cap"]), SENT_I, np.int32) if a["form"] == 1 else None
        state = np.full(a.get("state_elems", 10 * n + a["max_new"] + 1), SENT_I, np.int32) if a["form"] == 1 else None
        with pytest.raises(PceError):
            eng.selftest_decode_rules(a["form"], a["V"], logits, a["seqs"], a["sb"], a["eot"], a["ts"], a["mask"], out_tok, out_lp,
                                      pr if a["form"] == 0 else None, t_cap=a["t_cap"], max_new=a["max_new"], table=table, loop_state=state, **a["kw"])
        assert np.all(out_tok == SENT_I) and np.all(out_lp == SENT_F) and np.all(pr == SENT_F)
        assert table is None or (np.all(table == SENT_I) and np.all(state == SENT_I))

    refused(eot=vc.ts, ts=vc.eot)                                  # order of end-of-text and timestamp_begin
    refused(ts=vc.eot)
    refused(eot=-1)
    refused(ts=301)
    refused(kw=dict(temperature=-0.5))
    refused(kw=dict(temperature=float("nan")))
    refused(kw=dict(probe_token=300))
    big = Vocab(52225)
    refused(V=52225, eot=big.eot, ts=big.ts, mask=big.mask, ld=big.ld, seqs=[big.prompt])
    refused(ld=vc.ld - 128)                                        # logits shorter than [steps][n][ld]
    refused(mask=vc.mask[:299])
    refused(n_out=1)                                               # outputs shorter than n
    refused(seqs=[vc.prompt + [300]])                              # a token outside the vocabulary
    refused(t_cap=3)                                               # a sequence longer than t_cap
    refused(t_cap=449)
    refused(sb=0)
    refused(sb=5)                                                  # beyond a sequence's length (3)
    refused(sb=[3, 4])
    refused(steps=2)                                               # form 0 is one step
    loop = dict(form=1, t_cap=8, max_new=2, n_out=4)
    refused(**dict(loop, steps=3))                                 # more steps than max_new
    refused(**dict(loop, n_out=3))                                 # out_tok / out_lp shorter than [n][max_new]
    refused(**dict(loop, table_elems=15))
    refused(**dict(loop, state_elems=22))
    refused(**dict(loop, seqs=[vc.prompt * 3]))                    # a prompt longer than t_cap
    refused(**dict(loop, max_new=0, n_out=2))
