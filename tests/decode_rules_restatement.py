"""Float64 restatement of what turns a decoding step's logits into tokens: openai-whisper's logit filters (SuppressBlank, SuppressTokens,
ApplyTimestampRules with max_initial_timestamp_index and its probability-mass rule), GreedyDecoder's choice at temperature 0 and at a temperature
(the engine's counter-based Gumbel draw), the no_speech probe, and the table bookkeeping of the device-resident loop.  Written from decoding.py and
from the engine's documented draw (include/pce.h), not from the kernel's structure: plain numpy over one row at a time, plain Python over lists.
tests/test_decode_rules_host.py pins it to oracle/whisper_oracle.py and to Aligners/decoding.py; tests/test_gpu_decode_rules.py compares the
kernels with it."""
import numpy as np

NEG = -np.inf
M64 = (1 << 64) - 1
GOLD, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def logsumexp(x):
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return NEG
    m = x.max()
    if not np.isfinite(m):
        return m                                                   # all -inf (or +inf: not produced here)
    return float(m + np.log(np.exp(x - m).sum()))


def filtered(logits, tokens, sample_begin, eot, ts_begin, mask, max_initial=None):
    """The row after the filters, float64 [n_vocab] (-inf where suppressed), and the mass rule's margin logsumexp(timestamps) - max(text) it
    decided on (nan when one side is empty of finite values on both sides).  tokens: the sequence so far, prompt included; mask: uint8 [n_vocab],
    bit 0 = always suppressed, bit 1 = suppressed at the first sampled position."""
    x = np.array(logits, dtype=np.float64)
    mask = np.asarray(mask)
    seq = list(tokens[sample_begin:])
    if len(tokens) == sample_begin:                               # SuppressBlank
        x[(mask & 2) != 0] = NEG
    x[(mask & 1) != 0] = NEG                                      # SuppressTokens, <|notimestamps|>
    last_ts = len(seq) >= 1 and seq[-1] >= ts_begin               # ApplyTimestampRules: timestamps come in pairs, except before end-of-text
    pen_ts = len(seq) < 2 or seq[-2] >= ts_begin
    if last_ts:
        if pen_ts:
            x[ts_begin:] = NEG                                    # has to be non-timestamp
        else:
            x[:eot] = NEG                                         # cannot be normal text tokens
    stamps = [t for t in seq if t >= ts_begin]
    if stamps:                                                    # timestamps shouldn't decrease; forbid timestamp tokens smaller than the last
        last = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
        x[ts_begin:last] = NEG
    if len(tokens) == sample_begin:                               # suppress generating non-timestamp tokens at the beginning
        x[:ts_begin] = NEG
        if max_initial is not None:
            x[ts_begin + max_initial + 1:] = NEG
    # if sum of probability over timestamps is above any other token, sample timestamp (shift-invariant: the logits serve as log-probabilities)
    lse_ts, m_text = logsumexp(x[ts_begin:]), (x[:ts_begin].max() if ts_begin > 0 else NEG)
    margin = lse_ts - m_text if (np.isfinite(lse_ts) or np.isfinite(m_text)) else np.nan
    if lse_ts > m_text:
        x[:ts_begin] = NEG
    return x, margin


def log_softmax_at(x, i):
    return float(x[i] - logsumexp(x))


def choose(x, tokens, eot):
    """GreedyDecoder.update at temperature 0 on a filtered row -> (id, log-probability): first arg-max; a sequence whose last token is end-of-text
    stays there and adds nothing to sum_logprobs; a row without a finite candidate gives id 0, log-probability 0."""
    if len(tokens) and tokens[-1] == eot:
        return eot, 0.0
    if not np.isfinite(x.max()):
        return 0, 0.0
    i = int(np.argmax(x))
    return i, log_softmax_at(x, i)


def uniforms(seed, key, pos, ids):
    """The engine's uniform numbers for (seed, key, position) at the given ids, float64 [len(ids)]: two splitmix64 finalisers over the counter
    key << 40 ^ pos << 20 ^ id (64-bit wrap-around, key and pos as unsigned 32-bit), 23 bits + 1/2 over 2^23."""
    out = np.empty(len(ids), dtype=np.float64)
    k, p = int(key) & 0xFFFFFFFF, int(pos) & 0xFFFFFFFF
    for j, v in enumerate(ids):
        ctr = ((k << 40) & M64) ^ ((p << 20) & M64) ^ (int(v) & 0xFFFFFFFF)
        z = ((int(seed) & M64) + GOLD * ctr) & M64
        for r in range(2):
            if r:
                z = (z + GOLD) & M64
            z = ((z ^ (z >> 30)) * MIX1) & M64
            z = ((z ^ (z >> 27)) * MIX2) & M64
            z ^= z >> 31
        out[j] = ((z >> 41) + 0.5) / 8388608.0
    return out


def uniforms_np(seed, key, pos, n_vocab):
    """uniforms(seed, key, pos, range(n_vocab)) on numpy's wrapping uint64 arithmetic (the same integers; checked against it in the host tests)."""
    u64 = np.uint64
    k, p = int(key) & 0xFFFFFFFF, int(pos) & 0xFFFFFFFF
    base = ((k << 40) & M64) ^ ((p << 20) & M64)
    ctr = np.arange(n_vocab, dtype=np.uint64) ^ u64(base)         # (ids < 2^20 here; the xor is the general form all the same)
    with np.errstate(over="ignore"):
        z = u64(int(seed) & M64) + u64(GOLD) * ctr
        for r in range(2):
            if r:
                z = z + u64(GOLD)
            z = (z ^ (z >> u64(30))) * u64(MIX1)
            z = (z ^ (z >> u64(27))) * u64(MIX2)
            z = z ^ (z >> u64(31))
    return ((z >> u64(41)).astype(np.float64) + 0.5) / 8388608.0


def perturbed(x, temperature, seed, key, pos):
    """x / temperature - log(-log u) per id, float64 (-inf where x is), and the Gumbel terms g = log(-log u)"""
    u = uniforms_np(seed, key, pos, len(x))
    g = np.log(-np.log(u))
    with np.errstate(invalid="ignore"):
        p = np.where(np.isfinite(x), x / float(temperature) - g, NEG)
    return p, g


def sample(x, tokens, eot, temperature, seed, key):
    """GreedyDecoder.update at a temperature on a filtered row: one draw from softmax(x / temperature) as the arg-max of the perturbed values.
    -> (id, log-probability under the filtered UNSCALED distribution, gap of the perturbed values to the runner-up, perturbed, g)."""
    p, g = perturbed(x, temperature, seed, key, len(tokens))
    if not np.isfinite(x.max()):
        return (eot if len(tokens) and tokens[-1] == eot else 0), 0.0, np.inf, p, g
    i = int(np.argmax(p))
    rest = np.delete(p, i)
    gap = float(p[i] - rest.max()) if rest.size and np.isfinite(rest.max()) else np.inf
    if len(tokens) and tokens[-1] == eot:
        return eot, 0.0, gap, p, g
    return i, log_softmax_at(x, i), gap, p, g


def probe(logits, token):
    """softmax of the UNFILTERED row at one id"""
    x = np.asarray(logits, dtype=np.float64)
    return float(np.exp(x[token] - logsumexp(x)))


def loop(choices, prompts, t_cap, eot, max_new):
    """The device-resident loop's bookkeeping over scripted choices.  choices(step, seqs) -> [(id, log-probability)] for the current sequences
    (what the filters choose on each); prompts: lists of ids.  A sequence of t_cap tokens cannot take another: the choice is reported, the
    sequence stops and its last table entry reads end-of-text from then on.  -> dict of out_tok / out_lp [n][steps], table (lists, the live
    entries), len, ended, n_ended [steps], ct columns new token / key count / position [n], counter."""
    n = len(prompts)
    table = [list(p) for p in prompts]
    out_tok, out_lp, n_ended = [[] for _ in range(n)], [[] for _ in range(n)], []
    ended, tok, keys, posn = [0] * n, [0] * n, [0] * n, [0] * n
    step = 0
    while step < max_new:
        picks = choices(step, table)
        if picks is None:
            break
        cnt = 0
        for i, (t, lp) in enumerate(picks):
            out_tok[i].append(int(t)); out_lp[i].append(lp)
            L = len(table[i])
            if L < t_cap:
                table[i].append(int(t))
                keys[i], posn[i] = L + 1, L
            else:
                table[i][t_cap - 1] = eot
                keys[i], posn[i] = t_cap, t_cap - 1
            tok[i] = int(t)
            ended[i] = int(t == eot or L >= t_cap)
            cnt += ended[i]
        n_ended.append(cnt)
        step += 1
    return {"out_tok": out_tok, "out_lp": out_lp, "table": table, "len": [len(s) for s in table], "ended": ended, "n_ended": n_ended,
            "ct_tok": tok, "ct_keys": keys, "ct_pos": posn, "counter": step}
