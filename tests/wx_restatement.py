"""whisperX's alignment programme restated in numpy, straight from the specification above ``pce_wx_align`` in include/pce.h (itself restated
from the published source of whisperx 3.3.x, alignment.py: get_trellis / get_wildcard_emission / backtrack_beam).  The trellis lines are
pinned to torch's CPU operators in tests/test_wx_host.py; the back-track keeps parent pointers instead of copied paths, so that a clip of
4 100 frames stays fast.  Also the seeded cases the host and the device tests share."""
import numpy as np

INF = np.float32(np.inf)


def rowmax(e, blank):
    """max over v != blank of e[t][v], per frame (-inf when V = 1)."""
    m = np.array(e, dtype=np.float32, copy=True)
    m[:, blank] = -INF
    return m.max(axis=1)


def token_emissions(e, tok, blank):
    """wild(t, tok[j]) for every frame and token -> float32 [T, J]."""
    tok = np.asarray(tok, dtype=np.int64)
    out = e[:, np.maximum(tok, 0)].astype(np.float32)
    if (tok < 0).any():
        out[:, tok < 0] = rowmax(e, blank)[:, None]
    return out


def trellis(e, tok, blank):
    e = np.asarray(e, dtype=np.float32)
    T, J = e.shape[0], len(tok)
    tr = np.zeros((T, J), dtype=np.float32)
    tr[1:, 0] = np.cumsum(e[1:, blank].astype(np.float64)).astype(np.float32)        # fp64 accumulator in frame order, each prefix rounded
    tr[0, 1:] = -INF
    tr[(max(0, T - J + 1) if J >= 2 else 0):, 0] = INF                               # Python's trellis[-J + 1:, 0] = inf (-0: is the whole column)
    em = token_emissions(e, tok, blank)
    with np.errstate(invalid="ignore"):
        for t in range(T - 1):
            tr[t + 1, 1:] = np.maximum(tr[t, 1:] + e[t, blank], tr[t, :-1] + em[t, 1:])
    return tr


def backtrack(tr, e, tok, blank, W):
    """-> (path_tok int32 [T], path_lp float32 [T]) or None (no beam left)."""
    e = np.asarray(e, dtype=np.float32)
    T, J = tr.shape
    wm = rowmax(e, blank) if any(int(k) < 0 for k in tok) else None
    nodes = [(-1, J - 1, T - 1, e[T - 1, blank])]            # (parent node, token index, frame, lp)
    beams = [(J - 1, T - 1, tr[T - 1, J - 1], 0)]            # (j, t, score, node)
    while beams and beams[0][0] > 0:
        cands = []
        for j, t, _, node in beams:
            if t <= 0:
                continue
            stay = tr[t - 1, j]
            if not np.isinf(stay):
                nodes.append((node, j, t - 1, e[t - 1, blank]))
                cands.append((j, t - 1, stay, len(nodes) - 1))
            if j > 0:
                change = tr[t - 1, j - 1]
                if not np.isinf(change):
                    k = int(tok[j])                                                  # the emission belongs to the token being left
                    nodes.append((node, j - 1, t - 1, wm[t - 1] if k < 0 else e[t - 1, k]))
                    cands.append((j - 1, t - 1, change, len(nodes) - 1))
        beams = sorted(cands, key=lambda c: c[2], reverse=True)[:W]                   # stable: equal scores keep their emission order
    if not beams:
        return None
    j, t, _, node = beams[0]
    path_tok = np.empty(T, dtype=np.int32)
    path_lp = np.empty(T, dtype=np.float32)
    while node >= 0:
        node, jj, tt, lp = nodes[node]
        path_tok[tt] = jj
        path_lp[tt] = lp
    path_tok[:t] = j
    path_lp[:t] = e[:t, blank]
    return path_tok, path_lp


def align(e, tok, blank, W):
    """What ``ProsodyEngine.wx_align`` returns for one clip (status 0 OK, 1 EMPTY, 2 NO_PATH), with the trellis."""
    e = np.asarray(e, dtype=np.float32)
    T, J = e.shape[0], len(tok)
    if T == 0 or J == 0:
        return {"status": 1, "score": np.float32(np.nan), "path_tok": np.full(T, -1, np.int32), "path_lp": np.full(T, np.nan, np.float32),
                "trellis": np.zeros((T, J), np.float32)}
    tr = trellis(e, tok, blank)
    bt = backtrack(tr, e, tok, blank, W)
    if bt is None:
        return {"status": 2, "score": tr[T - 1, J - 1], "path_tok": np.full(T, -1, np.int32), "path_lp": np.full(T, np.nan, np.float32), "trellis": tr}
    return {"status": 0, "score": tr[T - 1, J - 1], "path_tok": bt[0], "path_lp": bt[1], "trellis": tr}


def log_softmax_rows(rng, T, V, quantised=False):
    """Seeded emissions: log-softmax rows, or rows quantised to multiples of 0.25 (scores then tie far beyond the structural ties)."""
    x = rng.standard_normal((T, V)) * 2.0
    lp = (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)
    if quantised:
        lp = (np.round(lp * 4.0) / 4.0).astype(np.float32)
    return lp


def make_case(seed, T, J, V, blank=0, quantised=False, wild=0.0, wild_at=()):
    """-> (e float32 [T, V], tok int32 [J]): tokens drawn from the whole vocabulary, a share ``wild`` of them (and the places ``wild_at``) wildcards."""
    rng = np.random.default_rng(seed)
    e = log_softmax_rows(rng, T, V, quantised)
    tok = rng.integers(0, V, size=J).astype(np.int32)
    if wild >= 1.0:
        tok[:] = -1
    elif wild > 0.0:
        tok[rng.random(J) < wild] = -1
    for j in wild_at:
        tok[j] = -1
    return e, tok
