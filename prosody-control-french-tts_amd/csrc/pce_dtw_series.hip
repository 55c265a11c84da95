// pce_dtw_series.hip -- dynamic time warping of pairs of fp64 series (the scoring step of Code/Pipeline/evaluate_voice.ipynb, cell 518367fb).
//
// The notebook aligns the voiced log-F0 frames of a recording with those of its synthesis through fastdtw(x, y, radius = 25) and reads the
// RMSE along the path.  The fastdtw package is third party and absent: its inner dynamic programme is restated here from the published
// source, parity unpinned.  For 1-D series with the package's default distance:
//     dt = |a[i] - b[j]|,   D[i+1][j+1] = min(D[i][j+1] + dt, D[i+1][j] + dt, D[i][j] + dt)
// the three SUMS compared in the order up, left, diagonal, the first minimum wins (Python's min over a tuple of candidates); D[0][0] = 0, the
// rest of row 0 / column 0 and every cell outside the row's column window [win_lo, win_hi) is +inf.  fp64 adds and compares only: a CPU
// restatement of these lines is bit-identical, path and distance.  (k_dtw of pce_align.hip is another recurrence: dense matrix, diagonal
// first, float32 accumulator.)
//
// The cost matrix is never formed.  A pair is cut into tiles: a stripe of DS_R rows (thread = row) x a chunk of DS_C columns.  Inside a tile
// the anti-diagonals sweep as in k_dtw; a thread keeps its left and diagonal neighbours in registers and takes the cell above from the
// row above through LDS (one fp64 per row, double buffered: one barrier per anti-diagonal).  The chunk of b, and the row above the stripe,
// sit in LDS; the stripe's last row overwrites that row in place and is flushed at the end.  Tiles hand over through HBM: boundary row s of a
// pair lives in the (s mod 3)-th of three row buffers (three, because the corner cell a tile starts from is read one launch after the
// neighbouring tile has written the next boundary into the same columns), the boundary column in one column buffer updated in place.
// Tiles with the same stripe + chunk index depend on nothing in their own launch: ONE LAUNCH PER BLOCK ANTI-DIAGONAL over all pairs of the
// group, the kernel boundary is the only synchronisation between workgroups (no flags, no grid barrier).
//
// With a window, a stripe visits the chunks that meet [min win_lo, max win_hi) of its rows; what a tile reads from a boundary is masked by
// the window of the row (column) that would have written it, so a boundary a skipped tile never wrote is never used.
//
// Trace: 2 bits per (row, anti-diagonal) of a tile, 16 anti-diagonals per 32-bit word, word (D / 16) * rows + row: every store of a wave is
// 256 contiguous bytes.  One lane per pair walks it back from (n - 1, m - 1) and writes the path from the END of the pair's output room
// towards its start, so it arrives in increasing order without a reversal pass; the host moves it to the front.
#include "pce_internal.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int DS_R = PCE_DTW_SERIES_ROWS, DS_C = PCE_DTW_SERIES_COLS;

struct DsPair {                 // one pair of the group in flight
    long long a_off, b_off;     // first element of its rows in a (and in win_lo / win_hi), of its columns in b
    long long row_off, col_off; // its three boundary rows [3][m + 1] / its boundary column [n + 1] (doubles; padded indices)
    long long tab_off;          // its tile table [stripes][chunks]: first trace word of the tile, -1 = not swept
    long long out_off;          // its room in path_i / path_j (n + m entries)
    int n, m, n_chunks, idx;    // idx: position in the caller's batch
};
struct DsTile { int pair, s, k, pad; long long tr_off; };

__global__ __launch_bounds__(DS_R) void k_dtw_series(const DsPair *__restrict__ pairs, const DsTile *__restrict__ tiles, const double *__restrict__ a,
                                                    const double *__restrict__ b, const int *__restrict__ win_lo, const int *__restrict__ win_hi,
                                                    double *rowbuf, double *colbuf, unsigned *__restrict__ trace, double *__restrict__ dist)
{
    __shared__ double s_b[DS_C];            // b of the chunk
    __shared__ double s_top[DS_C + 1];      // D of the row above the stripe at padded columns c0 .. c0 + Cw; becomes the stripe's last row
    __shared__ double s_up[2][DS_R];        // the previous anti-diagonal, by row
    const DsTile tl = tiles[blockIdx.x];
    const DsPair p = pairs[tl.pair];
    const int t = threadIdx.x, S = (int)blockDim.x;
    const int r0 = tl.s * DS_R, c0 = tl.k * DS_C;
    const int Rs = min(DS_R, p.n - r0), Cw = min(DS_C, p.m - c0);
    const double INF = __builtin_huge_val();
    const double *A = a + p.a_off, *B = b + p.b_off;
    const int *LO = win_lo ? win_lo + p.a_off : nullptr, *HI = win_lo ? win_hi + p.a_off : nullptr;
    const double *top = rowbuf + p.row_off + (long long)(tl.s % 3) * (p.m + 1);
    double *bot = rowbuf + p.row_off + (long long)((tl.s + 1) % 3) * (p.m + 1);
    double *col = colbuf + p.col_off;
    {
        // the row above the stripe: row 0 of the padded matrix for the first stripe, else what the stripe above left, masked by THAT row's window
        int plo = 0, phi = p.m;
        if (tl.s > 0 && LO) { plo = LO[r0 - 1]; phi = HI[r0 - 1]; }
        for (int x = t; x <= Cw; x += S) {
            const int pc = c0 + x;          // padded column: column pc - 1
            double v;
            if (tl.s == 0) v = pc == 0 ? 0.0 : INF;
            else v = (pc >= 1 && pc - 1 >= plo && pc - 1 < phi) ? top[pc] : INF;
            s_top[x] = v;
            if (x < Cw) s_b[x] = B[c0 + x];
        }
    }
    const int i = r0 + t;
    const bool row = t < Rs;
    double my_a = 0.0, left = INF, diag = INF;
    int lo = 0, hi = 0;
    if (row) {
        my_a = A[i];
        lo = LO ? LO[i] : 0; hi = LO ? HI[i] : p.m;
        if (tl.k > 0) {                     // column c0 - 1, written by the tile to the left: this row's and the row above's
            if (c0 - 1 >= lo && c0 - 1 < hi) left = col[i + 1];
            if (t > 0) {
                const int l1 = LO ? LO[i - 1] : 0, h1 = LO ? HI[i - 1] : p.m;
                if (c0 - 1 >= l1 && c0 - 1 < h1) diag = col[i];
            }
        }
    }
    __syncthreads();
    if (t == 0) diag = s_top[0];            // the corner (never from `col`: the stripe above rewrites that element in this very launch)
    unsigned acc = 0;
    unsigned *tr = trace + tl.tr_off;
    const int steps = Rs + Cw - 1;
    for (int D = 0; D < steps; D++) {
        const int jc = D - t;
        if (row && jc >= 0 && jc < Cw) {
            const double up = t == 0 ? s_top[jc + 1] : s_up[(D + 1) & 1][t - 1];
            const int j = c0 + jc;
            double cur = INF;
            if (j >= lo && j < hi) {
                const double dt = fabs(my_a - s_b[jc]);
                const double su = up + dt, sl = left + dt, sd = diag + dt;
                unsigned tt = 0u;
                cur = su;
                if (sl < cur) { cur = sl; tt = 1u; }
                if (sd < cur) { cur = sd; tt = 2u; }
                acc |= tt << (2 * (D & 15));
            }
            s_up[D & 1][t] = cur;
            if (t == Rs - 1) s_top[jc + 1] = cur;       // (thread 0 read this element at an earlier step, or just above when Rs == 1)
            diag = up; left = cur;
        }
        if ((D & 15) == 15 || D == steps - 1) {
            if (row) tr[(long long)(D >> 4) * Rs + t] = acc;
            acc = 0;
        }
        __syncthreads();
    }
    // `left` is the row's value in the chunk's last column
    if (row && tl.k + 1 < p.n_chunks) col[i + 1] = left;
    if (row && i == p.n - 1 && c0 + Cw == p.m) dist[p.idx] = left;
    if (r0 + Rs < p.n)
        for (int x = 1 + t; x <= Cw; x += S) bot[c0 + x] = s_top[x];
}

// one lane per pair; status: PCE_DTW_OK / PCE_DTW_NO_PATH (D[n][m] = +inf)
__global__ __launch_bounds__(64) void k_dtw_series_trace(const DsPair *__restrict__ pairs, int n_pairs, const long long *__restrict__ tiletab,
                                                         const unsigned *__restrict__ trace, const double *__restrict__ dist, int *__restrict__ path_i,
                                                         int *__restrict__ path_j, int *__restrict__ path_len, int *__restrict__ status)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= n_pairs) return;
    const DsPair p = pairs[q];
    if (!(dist[p.idx] < __builtin_huge_val())) { path_len[p.idx] = 0; status[p.idx] = PCE_DTW_NO_PATH; return; }
    const long long *tab = tiletab + p.tab_off;
    int *pi = path_i + p.out_off, *pj = path_j + p.out_off;
    const int room = p.n + p.m;
    int i = p.n - 1, j = p.m - 1, cnt = 0, st = PCE_DTW_OK;
    for (;;) {
        cnt++;
        pi[room - cnt] = i; pj[room - cnt] = j;
        if (i == 0 && j == 0) break;
        const int s = i / DS_R, t = i - s * DS_R, k = j / DS_C, D = t + (j - k * DS_C);
        const long long off = tab[(long long)s * p.n_chunks + k];
        if (off < 0 || cnt >= room) { st = PCE_DTW_NO_PATH; cnt = 0; break; }      // (a finite cell's chosen predecessor is finite: not reached)
        const int Rs = min(DS_R, p.n - s * DS_R);
        const unsigned tt = (trace[off + (long long)(D >> 4) * Rs + t] >> (2 * (D & 15))) & 3u;
        if (tt != 1u) i--;
        if (tt != 0u) j--;
        if (i < 0 || j < 0) { st = PCE_DTW_NO_PATH; cnt = 0; break; }
    }
    path_len[p.idx] = cnt; status[p.idx] = st;
}

struct PairPlan {
    int idx, n, m, n_stripes, n_chunks;
    std::vector<int> klo, khi;              // per stripe: chunks [klo, khi) are swept
    long long trace_words;
    double cells;
};

} // namespace

extern "C" {

int pce_dtw_series(pce_ctx *c, const double *a, const int64_t *a_off, const double *b, const int64_t *b_off, const int32_t *win_lo,
                   const int32_t *win_hi, int32_t batch, int32_t *path_i, int32_t *path_j, int32_t *path_len, double *dist, int32_t *status)
{
    if (!c || !a_off || !b_off || !path_len || !dist || !status || batch <= 0 || (win_lo == nullptr) != (win_hi == nullptr)) return PCE_E_INVALID;
    if (a_off[0] != 0 || b_off[0] != 0) return pce_fail(c, PCE_E_INVALID, "pce_dtw_series: offsets must start at 0");
    for (int32_t q = 0; q < batch; q++) {
        const int64_t n = a_off[q + 1] - a_off[q], m = b_off[q + 1] - b_off[q];
        if (n < 0 || m < 0) return pce_fail(c, PCE_E_INVALID, "pce_dtw_series: offsets of pair %d decrease", q);
        if (n > 0x3fffffff || m > 0x3fffffff) return pce_fail(c, PCE_E_LIMIT, "pce_dtw_series: pair %d is longer than 2^30 points", q);
    }
    const size_t na = (size_t)a_off[batch], nb = (size_t)b_off[batch], no = na + nb;
    if ((na && !a) || (nb && !b) || (no && (!path_i || !path_j))) return PCE_E_INVALID;
    for (size_t x = 0; x < na; x++) if (!std::isfinite(a[x])) return pce_fail(c, PCE_E_INVALID, "pce_dtw_series: a[%zu] is not finite", x);
    for (size_t x = 0; x < nb; x++) if (!std::isfinite(b[x])) return pce_fail(c, PCE_E_INVALID, "pce_dtw_series: b[%zu] is not finite", x);

    // plan every pair from its own n, m and window alone (what a pair computes does not depend on its batch)
    const long long budget_words = (long long)(c->sw.dtw_trace_budget / 4);
    std::vector<PairPlan> plans;
    for (int32_t q = 0; q < batch; q++) {
        const int n = (int)(a_off[q + 1] - a_off[q]), m = (int)(b_off[q + 1] - b_off[q]);
        path_len[q] = 0;
        if (n == 0 || m == 0) { dist[q] = std::nan(""); status[q] = PCE_DTW_EMPTY; continue; }
        dist[q] = HUGE_VAL; status[q] = PCE_DTW_NO_PATH;
        PairPlan pl;
        pl.idx = q; pl.n = n; pl.m = m; pl.n_stripes = (int)div_up(n, DS_R); pl.n_chunks = (int)div_up(m, DS_C);
        pl.klo.assign((size_t)pl.n_stripes, 0); pl.khi.assign((size_t)pl.n_stripes, 0);
        pl.trace_words = 0; pl.cells = 0.0;
        for (int s = 0; s < pl.n_stripes; s++) {
            const int r0 = s * DS_R, Rs = std::min(DS_R, n - r0);
            int mlo = 0, mhi = m;
            if (win_lo) {
                mlo = m; mhi = 0;
                for (int r = r0; r < r0 + Rs; r++) {
                    const int lo = win_lo[a_off[q] + r], hi = win_hi[a_off[q] + r];
                    if (lo < 0 || hi > m || lo > hi) return pce_fail(c, PCE_E_INVALID, "pce_dtw_series: window of row %d of pair %d is not 0 <= lo <= hi <= m", r, q);
                    if (lo < hi) { mlo = std::min(mlo, lo); mhi = std::max(mhi, hi); pl.cells += hi - lo; }
                }
            } else pl.cells += (double)Rs * m;
            if (mlo >= mhi) continue;
            pl.klo[(size_t)s] = mlo / DS_C; pl.khi[(size_t)s] = (mhi - 1) / DS_C + 1;
            for (int k = pl.klo[(size_t)s]; k < pl.khi[(size_t)s]; k++)
                pl.trace_words += div_up(Rs + std::min(DS_C, m - k * DS_C) - 1, 16) * Rs;
        }
        if (pl.trace_words > budget_words)
            return pce_fail(c, PCE_E_LIMIT, "pce_dtw_series: pair %d (%d x %d) needs %.1f MiB of trace, the budget is %.1f MiB (PCE_DTW_TRACE_MB)", q, n, m,
                            pl.trace_words * 4.0 / 1048576.0, c->sw.dtw_trace_budget / 1048576.0);
        plans.push_back(std::move(pl));
    }
    if (plans.empty()) return PCE_OK;

    PCE_HIP(c, hipSetDevice(c->device));
    pce_ctx::DtwSeries &w = c->ds;
    PCE_HIP(c, w.pi.reserve(sizeof(int) * no)); PCE_HIP(c, w.pj.reserve(sizeof(int) * no));
    PCE_UPLOAD(c, w.a, a, na); PCE_UPLOAD(c, w.b, b, nb);
    if (win_lo) { PCE_UPLOAD(c, w.lo, win_lo, na); PCE_UPLOAD(c, w.hi, win_hi, na); }
    // the host's initial values (inf / NaN, no path / empty, 0) are the device's too
    PCE_UPLOAD(c, w.dist, dist, (size_t)batch); PCE_UPLOAD(c, w.status, status, (size_t)batch); PCE_UPLOAD(c, w.len, path_len, (size_t)batch);

    // groups of consecutive pairs whose traces fit the budget together
    for (size_t g0 = 0; g0 < plans.size();) {
        size_t g1 = g0; long long words = 0;
        while (g1 < plans.size() && (g1 == g0 || words + plans[g1].trace_words <= budget_words)) words += plans[g1++].trace_words;
        std::vector<DsPair> dp(g1 - g0);
        std::vector<long long> tab;
        std::vector<DsTile> tiles;
        std::vector<int> diag_of;                        // block anti-diagonal of every tile
        long long row_words = 0, col_words = 0, tr = 0; int n_diag = 0; double cells = 0.0;
        for (size_t g = g0; g < g1; g++) {
            const PairPlan &pl = plans[g];
            DsPair &d = dp[g - g0];
            d.a_off = a_off[pl.idx]; d.b_off = b_off[pl.idx]; d.row_off = row_words; d.col_off = col_words; d.tab_off = (long long)tab.size();
            d.out_off = a_off[pl.idx] + b_off[pl.idx]; d.n = pl.n; d.m = pl.m; d.n_chunks = pl.n_chunks; d.idx = pl.idx;
            row_words += 3LL * (pl.m + 1); col_words += pl.n + 1; cells += pl.cells;
            tab.resize(tab.size() + (size_t)pl.n_stripes * (size_t)pl.n_chunks, -1LL);
            for (int s = 0; s < pl.n_stripes; s++) {
                const int Rs = std::min(DS_R, pl.n - s * DS_R);
                for (int k = pl.klo[(size_t)s]; k < pl.khi[(size_t)s]; k++) {
                    tab[(size_t)d.tab_off + (size_t)s * (size_t)pl.n_chunks + (size_t)k] = tr;
                    tiles.push_back(DsTile{(int)(g - g0), s, k, 0, tr}); diag_of.push_back(s + k);
                    n_diag = std::max(n_diag, s + k + 1);
                    tr += div_up(Rs + std::min(DS_C, pl.m - k * DS_C) - 1, 16) * Rs;
                }
            }
        }
        // tiles in launch order: counting sort by block anti-diagonal; the widest stripe of a launch sets its workgroup size
        std::vector<int> first((size_t)n_diag + 1, 0), threads((size_t)n_diag, 64);
        for (int L : diag_of) first[(size_t)L + 1]++;
        for (int L = 0; L < n_diag; L++) first[(size_t)L + 1] += first[(size_t)L];
        std::vector<DsTile> sorted(tiles.size());
        {
            std::vector<int> at(first.begin(), first.end() - 1);
            for (size_t x = 0; x < tiles.size(); x++) {
                const int L = diag_of[x];
                sorted[(size_t)at[(size_t)L]++] = tiles[x];
                const PairPlan &pl = plans[g0 + (size_t)tiles[x].pair];
                const int Rs = std::min(DS_R, pl.n - tiles[x].s * DS_R);
                threads[(size_t)L] = std::max(threads[(size_t)L], (int)div_up(Rs, 64) * 64);
            }
        }
        PCE_HIP(c, w.rows.reserve(sizeof(double) * (size_t)row_words)); PCE_HIP(c, w.cols.reserve(sizeof(double) * (size_t)col_words));
        PCE_HIP(c, w.trace.reserve(sizeof(unsigned) * (size_t)(tr + 1)));
        PCE_UPLOAD(c, w.pairs, dp); PCE_UPLOAD(c, w.tab, tab, 1); PCE_UPLOAD(c, w.tiles, sorted, 1);
        {
            KernelTimer t(c, PCE_K_DTW_SERIES, nullptr, cells);
            for (int L = 0; L < n_diag; L++) {
                const int cnt = first[(size_t)L + 1] - first[(size_t)L];
                if (!cnt) continue;
                hipLaunchKernelGGL(k_dtw_series, dim3((unsigned)cnt), dim3((unsigned)threads[(size_t)L]), 0, c->stream, w.pairs.as<DsPair>(),
                                   w.tiles.as<DsTile>() + first[(size_t)L], w.a.as<double>(), w.b.as<double>(), win_lo ? w.lo.as<int>() : nullptr,
                                   win_lo ? w.hi.as<int>() : nullptr, w.rows.as<double>(), w.cols.as<double>(), w.trace.as<unsigned>(), w.dist.as<double>());
            }
        }
        PCE_HIP(c, hipGetLastError());
        {
            KernelTimer t(c, PCE_K_DTW_SERIES_TRACE, nullptr, cells);
            hipLaunchKernelGGL(k_dtw_series_trace, dim3((unsigned)div_up((int64_t)dp.size(), 64)), dim3(64), 0, c->stream, w.pairs.as<DsPair>(), (int)dp.size(),
                               w.tab.as<long long>(), w.trace.as<unsigned>(), w.dist.as<double>(), w.pi.as<int>(), w.pj.as<int>(), w.len.as<int>(),
                               w.status.as<int>());
        }
        PCE_HIP(c, hipGetLastError());
        PCE_HIP(c, hipStreamSynchronize(c->stream));        // the group's host tables and the trace buffer are reused by the next group
        g0 = g1;
    }
    if (no) {
        PCE_FETCH(c, path_i, w.pi.p, no);
        PCE_FETCH(c, path_j, w.pj.p, no);
    }
    PCE_FETCH(c, path_len, w.len.p, (size_t)batch);
    PCE_FETCH(c, dist, w.dist.p, (size_t)batch);
    PCE_FETCH(c, status, w.status.p, (size_t)batch);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    // the walk wrote every path at the end of its room: move it to the front
    for (const PairPlan &pl : plans) {
        const size_t o = (size_t)(a_off[pl.idx] + b_off[pl.idx]), room = (size_t)pl.n + (size_t)pl.m, len = (size_t)path_len[pl.idx];
        if (len && len < room) {
            memmove(path_i + o, path_i + o + room - len, sizeof(int32_t) * len);
            memmove(path_j + o, path_j + o + room - len, sizeof(int32_t) * len);
        }
    }
    return PCE_OK;
}

} // extern "C"
