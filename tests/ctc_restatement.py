"""CPU restatement of the CTC forced alignment ``pce_ctc_align`` computes (a helper of the tests, not a test).

The recurrence is the CPU implementation of ``torchaudio.functional.forced_align``, restated in its plain form (every state of every
frame is computed; torchaudio's moving start / end window only leaves out states no complete path can visit) in numpy float32, written
for clarity.  Third party and absent: parity unpinned; ``tests/test_ctc_host.py`` checks it against exhaustive enumeration instead."""
import numpy as np

OK, EMPTY, TOO_SHORT, NO_PATH = 0, 1, 2, 3
NINF = np.float32(-np.inf)


def state_labels(targets, blank):
    """Labels of the 2 L + 1 states: blank at even states, targets[i // 2] at odd ones."""
    lab = np.full(2 * len(targets) + 1, blank, dtype=np.int64)
    lab[1::2] = targets
    return lab


def n_repeats(targets):
    t = np.asarray(targets)
    return int(np.sum(t[1:] == t[:-1])) if len(t) > 1 else 0


def forced_align(lp, targets, blank=0):
    """lp: [T, V] float32 log-probabilities -> dict(path, frame_score, tok_first, tok_last, score, status), as ``ProsodyEngine.ctc_align``."""
    lp = np.asarray(lp, dtype=np.float32)
    targets = np.asarray(targets, dtype=np.int64).reshape(-1)
    T, L = lp.shape[0], len(targets)
    none = dict(path=np.full(T, -1, np.int32), frame_score=np.full(T, np.nan, np.float32), tok_first=np.full(L, -1, np.int32),
                tok_last=np.full(L, -1, np.int32), score=np.float32(np.nan))
    if L == 0 or T == 0:
        return dict(none, status=EMPTY)
    if np.any(targets < 0) or np.any(targets >= lp.shape[1]) or np.any(targets == blank):
        raise ValueError("a target outside the vocabulary, or the blank")
    if T < L + n_repeats(targets):
        return dict(none, status=TOO_SHORT)
    S = 2 * L + 1
    lab = state_labels(targets, blank)
    skip = np.zeros(S, dtype=bool)                       # the states that may take alpha[i - 2]
    for i in range(3, S, 2):
        skip[i] = targets[i // 2] != targets[i // 2 - 1]
    alpha = np.full(S, NINF, dtype=np.float32)
    alpha[0] = lp[0, blank]
    alpha[1] = lp[0, targets[0]]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        x0 = alpha
        x1 = np.concatenate(([NINF], alpha[:-1])).astype(np.float32)
        x2 = np.where(skip, np.concatenate(([NINF, NINF], alpha[:-2])), NINF).astype(np.float32)
        take2 = (x2 > x1) & (x2 > x0)
        take1 = ~take2 & (x1 > x0) & (x1 > x2)
        chosen = np.where(take2, x2, np.where(take1, x1, x0)).astype(np.float32)
        back[t] = np.where(take2, 2, np.where(take1, 1, 0))
        with np.errstate(invalid="ignore"):
            alpha = (chosen + lp[t, lab]).astype(np.float32)
    i = S - 1 if alpha[S - 1] > alpha[S - 2] else S - 2
    score = np.float32(alpha[i])
    if score == NINF or np.isnan(score):
        return dict(none, score=score, status=NO_PATH)
    states = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = i
        i -= int(back[t, i])
    path = lab[states].astype(np.int32)
    first = np.full(L, -1, np.int32); last = np.full(L, -1, np.int32)
    for t, s in enumerate(states):
        if s & 1:
            if first[s // 2] < 0:
                first[s // 2] = t
            last[s // 2] = t
    return dict(path=path, frame_score=lp[np.arange(T), path].astype(np.float32), tok_first=first, tok_last=last, score=score, status=OK)


def path_score(lp, path):
    """The float32 sum of a path's emissions in frame order (what alpha accumulates along it)."""
    s = np.float32(lp[0, path[0]])
    for t in range(1, len(path)):
        s = np.float32(s + lp[t, path[t]])
    return s


def valid_state_paths(T, targets):
    """Every state sequence CTC admits: starts in state 0 or 1, ends in 2 L - 1 or 2 L, stays, advances by one, or skips a blank between
    two DIFFERENT targets."""
    L = len(targets); S = 2 * L + 1
    out = []

    def grow(seq):
        if len(seq) == T:
            if seq[-1] >= S - 2:
                out.append(tuple(seq))
            return
        i = seq[-1]
        for j in (i, i + 1, i + 2):
            if j >= S or (j == i + 2 and not (j & 1 and targets[j // 2] != targets[j // 2 - 1])):
                continue
            grow(seq + [j])

    for s0 in (0, 1):
        if s0 < S:
            grow([s0])
    return out


def merge_repeats(path):
    """Runs of equal labels -> [(label, first_frame, last_frame)], the last frame inclusive."""
    segs = []
    for t, lab in enumerate(path):
        if segs and segs[-1][0] == int(lab):
            segs[-1][2] = t
        else:
            segs.append([int(lab), t, t])
    return [tuple(s) for s in segs]


def same_result(a, b):
    """Exact equality of two result dicts: integers equal, floats equal in their bits (NaN matches NaN)."""
    def bits(x):
        x = np.atleast_1d(np.asarray(x, dtype=np.float32))
        return np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32))
    return (a["status"] == b["status"] and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("path", "tok_first", "tok_last"))
            and np.array_equal(bits(a["frame_score"]), bits(b["frame_score"])) and np.array_equal(bits(a["score"]), bits(b["score"])))
