"""What ``difflib.SequenceMatcher(None, a, b, autojunk).ratio()`` computes, restated as the dynamic programme ``k_seqmatch`` runs
(include/pce.h states the same five rules), and the alignment DP of "Compare Breaks" (Code/audioPipeline.py:973-998), stated as k_seqmatch_align runs it: a 2-bit trace, walked back.

Plain Python, no device: tests/test_compare_breaks_host.py pins this file to stdlib ``difflib``; the GPU tests compare the kernels
with ``difflib`` itself and use the DP below on ``difflib`` ratios."""
from collections import Counter


def popular_flags(b, autojunk=True):
    """Rule 1: with autojunk and len(b) >= 200, an element occurring more than len(b) // 100 + 1 times in b is popular."""
    n = len(b)
    if not autojunk or n < 200:
        return [False] * n
    count = Counter(b)
    ntest = n // 100 + 1
    return [count[x] > ntest for x in b]


def find_longest_match(a, b, pop, alo, ahi, blo, bhi):
    """Rules 2 and 3 -> (i, j, k)."""
    besti, bestj, bestsize = alo, blo, 0
    prev = [0] * (bhi - blo + 1)                            # prev[x + 1] = run length ending at (i - 1, blo + x); prev[0]: nothing continues across blo
    for i in range(alo, ahi):
        cur = [0] * (bhi - blo + 1)
        for j in range(blo, bhi):
            if b[j] == a[i] and not pop[j]:
                k = cur[j - blo + 1] = prev[j - blo] + 1
                if k > bestsize:                            # replaced on > only: largest k, then smallest i, then smallest j
                    besti, bestj, bestsize = i - k + 1, j - k + 1, k
        prev = cur
    while besti > alo and bestj > blo and a[besti - 1] == b[bestj - 1]:
        besti, bestj, bestsize = besti - 1, bestj - 1, bestsize + 1
    while besti + bestsize < ahi and bestj + bestsize < bhi and a[besti + bestsize] == b[bestj + bestsize]:
        bestsize += 1
    return besti, bestj, bestsize


def matches(a, b, autojunk=True, stats=None):
    """Rule 4: the summed sizes of the matching blocks.  ``stats`` (a dict) receives the deepest stack, the block count and the cells swept."""
    pop = popular_flags(b, autojunk)
    stack = [(0, len(a), 0, len(b))]
    total, deepest, blocks, cells = 0, 1, 0, 0
    while stack:
        alo, ahi, blo, bhi = stack.pop()
        cells += (ahi - alo) * (bhi - blo)
        i, j, k = find_longest_match(a, b, pop, alo, ahi, blo, bhi)
        if k:
            total += k; blocks += 1
            if alo < i and blo < j:
                stack.append((alo, i, blo, j))
            if i + k < ahi and j + k < bhi:
                stack.append((i + k, ahi, j + k, bhi))
            deepest = max(deepest, len(stack))
    if stats is not None:
        stats["deepest"], stats["blocks"], stats["cells"] = deepest, blocks, cells
    return total


def ratio(a, b, autojunk=True):
    """Rule 5."""
    length = len(a) + len(b)
    return 2.0 * matches(a, b, autojunk) / length if length else 1.0


TRACE_DIAGONAL, TRACE_UP, TRACE_LEFT = 0, 1, 2


def align(sim, n, m):
    """The alignment DP of "Compare Breaks" on a matrix of ratios ``sim[i][j]`` -> the diagonal steps [(i, j), ...], ascending.
    score(i, j) over the first i rows and j columns, 0 on either border: the row above if it is >= both the column to the left and
    score(i-1, j-1) + sim; else the column to the left if it is >= that sum; else the sum, a diagonal step."""
    trace = [bytearray(m) for _ in range(n)]
    above = [0.0] * (m + 1)
    for i in range(n):
        row = [0.0]
        for j in range(m):
            summed = above[j] + sim[i][j]
            if above[j + 1] >= row[j] and above[j + 1] >= summed:
                row.append(above[j + 1]); trace[i][j] = TRACE_UP
            elif row[j] >= summed:
                row.append(row[j]); trace[i][j] = TRACE_LEFT
            else:
                row.append(summed); trace[i][j] = TRACE_DIAGONAL
        above = row
    out = []
    i, j = n, m
    while i and j:
        step = trace[i - 1][j - 1]
        i -= step != TRACE_LEFT
        j -= step != TRACE_UP
        if step == TRACE_DIAGONAL:
            out.append((i, j))
    return out[::-1]
