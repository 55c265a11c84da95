// pce_seqmatch.hip -- difflib.SequenceMatcher(None, a, b).ratio() for batches of string pairs, and the fuzzy alignment built on it.
//
// "Compare Breaks" (Code/audioPipeline.py:895-1074) aligns every speech chunk of BDD_syntagme_for_synth.csv with the speech blocks of
// OUT.TextGrid: sim() (:970-971) is SequenceMatcher.ratio() of the two normalised strings, called for all n x m pairs inside the
// alignment DP (:973-998).  Both halves are exact: the matching is integer, the ratio one exact product and one correctly rounded fp64
// division, the DP fp64 adds and >= comparisons in a fixed order.  What SequenceMatcher computes (include/pce.h states the rules):
//   popular     with autojunk and len(b) >= 200, an element occurring more than len(b) / 100 + 1 times in b never starts or continues a
//               run (it is not junk: the extension below runs over it).  A count per distinct element of b: the host wrapper makes the
//               flags once per b string.
//   longest     over i in [alo, ahi) ascending and the non-popular j in [blo, bhi) with b[j] == a[i] ascending, k = len[i-1][j-1] + 1
//               (0 across blo); the best run is replaced on k > best only: largest k, then smallest i, then smallest j.
//   extension   left while a[i-1] == b[j-1] inside the range, then right.
//   blocks      a LIFO stack of ranges from (0, la, 0, lb); a match of k > 0 adds k and pushes what lies left and right of it.
//
// k_seqmatch: one WAVE per pair, SM_WAVES pairs in flight per workgroup, a fixed grid of waves striding over the pairs (so the scratch
// below is per wave, not per pair).  The lanes take 64-column chunks of the current range of b; the rows of a are swept with the previous
// row of run lengths kept per wave, updated in place from the last chunk to the first (a cell needs its left neighbour's OLD value).  A
// range of at most SM_ROW_CAP columns keeps the row in LDS, a wider one in a global row of the wave (one device-scope fence per row of a).
// The stack keeps SM_STACK_LDS ranges in LDS and the rest in a global spill of min(max la, max lb) + 1 entries per wave, written and read
// by lane 0 alone.  No barrier: the waves of a workgroup never meet.
//
// k_seqmatch_align: the DP of :973-998 over the n x m matched totals, as k_nw (pce_align.hip) sweeps its matrix: one workgroup, thread =
// row, anti-diagonals, the two previous diagonals in LDS, stripes of 1 024 rows handed over through a global row; a 2-bit trace packed
// 16 columns to a word (a word belongs to one row, hence to one thread), walked back by one lane.
#include "pce_internal.h"
#include <algorithm>
#include <unordered_map>
#include <vector>

namespace {

constexpr int SM_ROW_CAP = PCE_SEQMATCH_ROW_LDS;     // columns of a range whose row of run lengths lives in LDS
constexpr int SM_STACK_LDS = PCE_SEQMATCH_STACK_LDS; // ranges of the stack kept in LDS
constexpr int SM_WAVES = 4;                          // pairs in flight per workgroup
constexpr int AL_ROWS = 1024;                        // rows of one stripe of the alignment DP

// the order in which find_longest_match keeps a run that ends at (i, j): longer, then earlier in a, then earlier in b
__device__ __forceinline__ bool sm_better(int k, int i, int j, int K, int I, int J) { return k > K || (k == K && (i < I || (i == I && j < J))); }

// rows [alo, ahi) x columns [blo, bhi): per lane the best run end (k, i, j) it has seen.  `row` holds the run lengths of the previous
// row of a, indexed by column - blo; in_global: it lives in global memory, where another lane's store needs a fence to be seen.
__device__ __forceinline__ void sm_sweep(const unsigned *__restrict__ A, const unsigned *__restrict__ B, const unsigned char *__restrict__ P, int alo,
                                         int ahi, int blo, int bhi, int lane, int *row, bool in_global, int &bk, int &bi, int &bj)
{
    const int W = bhi - blo, n_chunks = (W + 63) >> 6;
    for (int i = alo; i < ahi; i++) {
        const unsigned ai = A[i];
        for (int ch = n_chunks - 1; ch >= 0; ch--) {       // descending: row[x - 1] still holds the previous row's value
            const int x = (ch << 6) + lane;
            // read phase, then write phase: lane x - 1 stores row[x - 1] in this same chunk, so every lane must have loaded before any
            // lane stores.  The 64 lanes of a wave run in lockstep, which orders the two phases in hardware; the wavefront fence and the
            // wave barrier (no instruction either) keep the compiler from moving a load or a store across the boundary.
            int left = 0;
            if (x < W && x > 0 && i > alo) left = row[x - 1];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (x < W) {
                const int j = blo + x;
                const int k = (B[j] == ai && !P[j]) ? left + 1 : 0;
                row[x] = k;
                if (k > 0 && sm_better(k, i, j, bk, bi, bj)) { bk = k; bi = i; bj = j; }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (in_global) __threadfence();
    }
}

__global__ __launch_bounds__(64 * SM_WAVES) void k_seqmatch(const unsigned *__restrict__ a_chars, const long long *__restrict__ a_off,
                                                          const unsigned *__restrict__ b_chars, const long long *__restrict__ b_off, int n_b,
                                                          const unsigned char *__restrict__ b_pop, const int *__restrict__ pair_a,
                                                          const int *__restrict__ pair_b, long long n_pairs, int *__restrict__ rows,
                                                          long long row_stride, int4 *__restrict__ spill, long long spill_stride,
                                                          int *__restrict__ out, unsigned long long *__restrict__ cells_out)
{
    __shared__ int row_lds[SM_WAVES][SM_ROW_CAP];
    __shared__ int4 stack_lds[SM_WAVES][SM_STACK_LDS];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));     // (wave-uniform: scalar loop control)
    const long long wave = (long long)blockIdx.x * SM_WAVES + w, n_waves = (long long)gridDim.x * SM_WAVES;
    int *row_g = rows + wave * row_stride;
    int4 *spill_g = spill + wave * spill_stride;
    unsigned long long cells = 0;
    for (long long p = wave; p < n_pairs; p += n_waves) {
        const long long ia = pair_a ? (long long)pair_a[p] : p / n_b, ib = pair_b ? (long long)pair_b[p] : p % n_b;
        const long long a0 = a_off[ia], b0 = b_off[ib];
        const int la = __builtin_amdgcn_readfirstlane((int)(a_off[ia + 1] - a0)), lb = __builtin_amdgcn_readfirstlane((int)(b_off[ib + 1] - b0));
        const unsigned *A = a_chars + a0, *B = b_chars + b0;
        const unsigned char *P = b_pop + b0;
        int matches = 0, sp = 0;
        if (la > 0 && lb > 0) { if (lane == 0) stack_lds[w][0] = make_int4(0, la, 0, lb); sp = 1; }
        while (sp > 0) {
            sp--;
            int4 r = make_int4(0, 0, 0, 0);
            if (lane == 0) r = sp < SM_STACK_LDS ? stack_lds[w][sp] : spill_g[sp - SM_STACK_LDS];       // lane 0 wrote it, lane 0 reads it
            const int alo = __builtin_amdgcn_readfirstlane(r.x), ahi = __builtin_amdgcn_readfirstlane(r.y);
            const int blo = __builtin_amdgcn_readfirstlane(r.z), bhi = __builtin_amdgcn_readfirstlane(r.w);
            cells += (unsigned long long)(ahi - alo) * (unsigned long long)(bhi - blo);
            int bk = 0, bi = alo, bj = blo;
            if (bhi - blo <= SM_ROW_CAP) sm_sweep(A, B, P, alo, ahi, blo, bhi, lane, row_lds[w], false, bk, bi, bj);
            else sm_sweep(A, B, P, alo, ahi, blo, bhi, lane, row_g, true, bk, bi, bj);
            for (int s = 1; s < 64; s <<= 1) {
                const int ok = __shfl_xor(bk, s, 64), oi = __shfl_xor(bi, s, 64), oj = __shfl_xor(bj, s, 64);
                if (sm_better(ok, oi, oj, bk, bi, bj)) { bk = ok; bi = oi; bj = oj; }
            }
            int k = __builtin_amdgcn_readfirstlane(bk);
            int i = __builtin_amdgcn_readfirstlane(bi), j = __builtin_amdgcn_readfirstlane(bj);
            if (k > 0) { i -= k - 1; j -= k - 1; }                             // run end -> run start (k == 0: (alo, blo))
            while (i > alo && j > blo && A[i - 1] == B[j - 1]) { i--; j--; k++; }
            while (i + k < ahi && j + k < bhi && A[i + k] == B[j + k]) k++;
            if (k > 0) {
                matches += k;
                if (alo < i && blo < j) {
                    if (lane == 0) { const int4 v = make_int4(alo, i, blo, j); if (sp < SM_STACK_LDS) stack_lds[w][sp] = v; else spill_g[sp - SM_STACK_LDS] = v; }
                    sp++;
                }
                if (i + k < ahi && j + k < bhi) {
                    if (lane == 0) { const int4 v = make_int4(i + k, ahi, j + k, bhi); if (sp < SM_STACK_LDS) stack_lds[w][sp] = v; else spill_g[sp - SM_STACK_LDS] = v; }
                    sp++;
                }
            }
        }
        if (lane == 0) out[p] = matches;
    }
    if (lane == 0) cells_out[wave] = cells;
}

// dp[i][j] over the matched totals M [n][m]: sim = 2.0 * M / (la_i + lb_j) (1.0 for two empty strings), match = dp[i-1][j-1] + sim,
// up if dp[i-1][j] >= dp[i][j-1] && dp[i-1][j] >= match, else left if dp[i][j-1] >= match, else diagonal (:978-988); dp[0][.] = dp[.][0] = 0.
// trace: 0 diagonal, 1 up, 2 left; 16 columns of a row per 32-bit word, tr_ld words per row.
__global__ __launch_bounds__(AL_ROWS) void k_seqmatch_align(const int *__restrict__ M, const long long *__restrict__ a_off, int n,
                                                           const long long *__restrict__ b_off, int m, double *__restrict__ sim_out,
                                                           unsigned *__restrict__ trace, long long tr_ld, double *__restrict__ rows,
                                                           int *__restrict__ match_a, int *__restrict__ match_b, int *__restrict__ n_matches)
{
    __shared__ double diag[3][AL_ROWS + 1];
    const int t = threadIdx.x, S = (int)blockDim.x;
    // stripes of S rows as in k_nw: local diagonal D holds dp[r0 + lr][D - lr] at index lr, thread t owns local row lr = t + 1, index 0 is the row
    // above the stripe: zeros for the first stripe, the previous stripe's last row (handed over through `top`) for the others
    double *top = rows, *bot = rows + (m + 1);              // only touched when n > S
    for (int r0 = 0; r0 < n; r0 += S) {
        const int R = min(S, n - r0), lr = t + 1, gr = r0 + lr;
        const bool first = r0 == 0, more = r0 + S < n;
        const long long la = t < R ? a_off[gr] - a_off[gr - 1] : 0;
        if (t == 0) diag[0][0] = 0.0;                      // dp[r0][0]
        double tv = (t == 0 && m >= 1 && !first) ? top[1] : 0.0;          // dp[r0][D] for the coming diagonal, fetched one step ahead
        unsigned tw = 0u;
        __syncthreads();
        for (int D = 1; D <= R + m; D++) {
            double *cur = diag[D % 3]; const double *p1 = diag[(D + 2) % 3], *p2 = diag[(D + 1) % 3];
            const int c = D - lr;
            if (t < R) {
                if (c >= 1 && c <= m) {
                    const size_t cell = (size_t)(gr - 1) * (size_t)m + (size_t)(c - 1);
                    const long long T = la + (b_off[c] - b_off[c - 1]);
                    const double sim = T == 0 ? 1.0 : 2.0 * (double)M[cell] / (double)T;
                    if (sim_out) sim_out[cell] = sim;
                    const double up = p1[lr - 1], lf = p1[lr], match = p2[lr - 1] + sim;
                    double best; unsigned tt;
                    if (up >= lf && up >= match) { best = up; tt = 1u; }
                    else if (lf >= match) { best = lf; tt = 2u; }
                    else { best = match; tt = 0u; }
                    cur[lr] = best;
                    tw |= tt << (2 * ((c - 1) & 15));
                    if (((c - 1) & 15) == 15 || c == m) { trace[(size_t)(gr - 1) * (size_t)tr_ld + (size_t)((c - 1) >> 4)] = tw; tw = 0u; }
                    if (more && lr == R) bot[c] = best;    // the stripe's last row: the next stripe's boundary
                } else if (c == 0) {
                    cur[lr] = 0.0;                         // dp[gr][0]
                }
            }
            if (t == 0 && D <= m) { cur[0] = tv; if (D + 1 <= m) tv = first ? 0.0 : top[D + 1]; }       // dp[r0][D]
            __syncthreads();
        }
        if (more) { __threadfence(); __syncthreads(); double *x = top; top = bot; bot = x; }
    }
    __threadfence();
    __syncthreads();
    if (t == 0) {
        int i = n, j = m, k = 0;
        while (i > 0 && j > 0) {                           // (:992-998)
            const unsigned tt = (trace[(size_t)(i - 1) * (size_t)tr_ld + (size_t)((j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u;
            if (tt == 0u) { match_a[k] = i - 1; match_b[k] = j - 1; k++; i--; j--; }
            else if (tt == 1u) i--;
            else j--;
        }
        for (int x = 0, z = k - 1; x < z; x++, z--) {
            const int ta = match_a[x], tb = match_b[x]; match_a[x] = match_a[z]; match_b[x] = match_b[z]; match_a[z] = ta; match_b[z] = tb;
        }
        *n_matches = k;
    }
}

// offsets of a string table: [n + 1], from 0, not decreasing, every string shorter than 2^30 elements
int sm_check_table(pce_ctx *c, const char *who, const char *which, const uint32_t *chars, const int64_t *off, int32_t n, int64_t *max_len)
{
    if (off[0] != 0) return pce_fail(c, PCE_E_INVALID, "%s: %s offsets must start at 0", who, which);
    int64_t mx = 0;
    for (int32_t s = 0; s < n; s++) {
        const int64_t len = off[s + 1] - off[s];
        if (len < 0) return pce_fail(c, PCE_E_INVALID, "%s: %s offsets decrease at string %d", who, which, s);
        if (len > 0x3fffffff) return pce_fail(c, PCE_E_LIMIT, "%s: %s string %d has 2^30 elements or more", who, which, s);
        if (len > mx) mx = len;
    }
    if (off[n] && !chars) return pce_fail(c, PCE_E_INVALID, "%s: %s table has offsets but no elements", who, which);
    *max_len = mx;
    return PCE_OK;
}

// difflib's popular elements of every b string (autojunk: len >= 200, more than len / 100 + 1 occurrences): one flag per element of the table
void sm_popular_flags(const uint32_t *chars, const int64_t *off, int32_t n, bool autojunk, std::vector<unsigned char> &flags)
{
    flags.assign((size_t)off[n] + 1, 0);
    if (!autojunk) return;
    std::unordered_map<uint32_t, int64_t> count;
    for (int32_t s = 0; s < n; s++) {
        const int64_t len = off[s + 1] - off[s];
        if (len < 200) continue;
        const int64_t ntest = len / 100 + 1;
        count.clear();
        for (int64_t x = off[s]; x < off[s + 1]; x++) count[chars[x]]++;
        for (int64_t x = off[s]; x < off[s + 1]; x++) flags[(size_t)x] = count[chars[x]] > ntest ? 1 : 0;
    }
}

// everything both entry points share: the tables go up, k_seqmatch runs, the matched totals stay on the device in d_out [n_pairs]
// (pop_host: the flags on their way up; they live until the caller has synchronised)
struct SmDevice { DevBuf a, b, ao, bo, pop, pa, pb, rows, spill, cells, out; std::vector<unsigned char> pop_host; };

int sm_run(pce_ctx *c, const char *who, const uint32_t *a_chars, const int64_t *a_off, int32_t n_a, const uint32_t *b_chars, const int64_t *b_off,
           int32_t n_b, const int32_t *pair_a, const int32_t *pair_b, int64_t n_pairs, int32_t autojunk, SmDevice &d)
{
    int64_t max_la = 0, max_lb = 0;
    PCE_TRY(sm_check_table(c, who, "a", a_chars, a_off, n_a, &max_la));
    PCE_TRY(sm_check_table(c, who, "b", b_chars, b_off, n_b, &max_lb));
    if (pair_a) {
        for (int64_t p = 0; p < n_pairs; p++)
            if (pair_a[p] < 0 || pair_a[p] >= n_a || pair_b[p] < 0 || pair_b[p] >= n_b)
                return pce_fail(c, PCE_E_INVALID, "%s: pair %lld names string (%d, %d) of tables of %d and %d", who, (long long)p, pair_a[p], pair_b[p], n_a, n_b);
    }
    if (n_pairs == 0) return PCE_OK;
    // a fixed grid of waves strides over the pairs: scratch per wave, sized for the longest strings of the tables
    const int64_t row_stride = max_lb > SM_ROW_CAP ? max_lb : 0, spill_stride = std::min(max_la, max_lb) + 1;
    const int64_t per_wave = row_stride * (int64_t)sizeof(int) + spill_stride * (int64_t)sizeof(int4);
    int64_t groups = std::min<int64_t>(div_up(n_pairs, SM_WAVES), (int64_t)std::max(c->cu_count, 1) * 8);
    while (groups > 1 && groups * SM_WAVES * per_wave > PCE_SEQMATCH_SCRATCH_MAX) groups = (groups + 1) / 2;
    if (SM_WAVES * per_wave > PCE_SEQMATCH_SCRATCH_MAX)
        return pce_fail(c, PCE_E_LIMIT, "%s: strings of %lld and %lld elements need %lld bytes of scratch per workgroup, at most %lld", who,
                        (long long)max_la, (long long)max_lb, (long long)(SM_WAVES * per_wave), (long long)PCE_SEQMATCH_SCRATCH_MAX);
    std::vector<unsigned char> &pop = d.pop_host;
    sm_popular_flags(b_chars, b_off, n_b, autojunk != 0, pop);
    const size_t na = (size_t)a_off[n_a], nb = (size_t)b_off[n_b];
    const size_t waves = (size_t)groups * SM_WAVES;
    PCE_HIP(c, d.rows.reserve(sizeof(int) * (waves * (size_t)row_stride + 1))); PCE_HIP(c, d.spill.reserve(sizeof(int4) * waves * (size_t)spill_stride));
    PCE_HIP(c, d.cells.reserve(sizeof(unsigned long long) * waves)); PCE_HIP(c, d.out.reserve(sizeof(int) * (size_t)n_pairs));
    PCE_UPLOAD(c, d.a, a_chars, na, 1); PCE_UPLOAD(c, d.b, b_chars, nb, 1);
    PCE_UPLOAD(c, d.ao, a_off, (size_t)n_a + 1); PCE_UPLOAD(c, d.bo, b_off, (size_t)n_b + 1); PCE_UPLOAD(c, d.pop, pop);
    if (pair_a) { PCE_UPLOAD(c, d.pa, pair_a, (size_t)n_pairs); PCE_UPLOAD(c, d.pb, pair_b, (size_t)n_pairs); }
    {
        KernelTimer t(c, PCE_K_SEQMATCH);
        hipLaunchKernelGGL(k_seqmatch, dim3((unsigned)groups), dim3(64 * SM_WAVES), 0, c->stream, d.a.as<unsigned>(), d.ao.as<long long>(),
                           d.b.as<unsigned>(), d.bo.as<long long>(), (int)n_b, d.pop.as<unsigned char>(), pair_a ? d.pa.as<int>() : nullptr,
                           pair_a ? d.pb.as<int>() : nullptr, (long long)n_pairs, d.rows.as<int>(), (long long)row_stride, d.spill.as<int4>(),
                           (long long)spill_stride, d.out.as<int>(), d.cells.as<unsigned long long>());
    }
    PCE_HIP(c, hipGetLastError());
    if (c->prof) {                                         // the work count of the launch: cells its waves swept, recursion included
        std::vector<unsigned long long> cells(waves);
        PCE_FETCH(c, cells.data(), d.cells.p, waves);
        PCE_HIP(c, hipStreamSynchronize(c->stream));
        double sum = 0.0;
        for (unsigned long long v : cells) sum += (double)v;
        c->prof_flops[PCE_K_SEQMATCH] += sum;
    }
    return PCE_OK;
}

int sm_check_args(pce_ctx *c, const char *who, const int64_t *a_off, int32_t n_a, const int64_t *b_off, int32_t n_b, int64_t n_pairs)
{
    if (!c) return PCE_E_INVALID;
    if (!a_off || !b_off || n_a < 0 || n_b < 0 || n_pairs < 0) return pce_fail(c, PCE_E_INVALID, "%s: null offsets or a negative count", who);
    if (n_pairs > PCE_SEQMATCH_MAX_PAIRS) return pce_fail(c, PCE_E_LIMIT, "%s: %lld pairs, at most %lld in one call", who, (long long)n_pairs, (long long)PCE_SEQMATCH_MAX_PAIRS);
    return PCE_OK;
}

} // namespace

extern "C" {

int pce_seqmatch(pce_ctx *c, const uint32_t *a_chars, const int64_t *a_off, int32_t n_a, const uint32_t *b_chars, const int64_t *b_off, int32_t n_b,
                 const int32_t *pair_a, const int32_t *pair_b, int64_t n_pairs, int32_t autojunk, int32_t *out_matches)
{
    PCE_TRY(sm_check_args(c, "pce_seqmatch", a_off, n_a, b_off, n_b, n_pairs));
    if ((pair_a == nullptr) != (pair_b == nullptr)) return pce_fail(c, PCE_E_INVALID, "pce_seqmatch: pair_a and pair_b go together");
    if (!pair_a && n_pairs != (int64_t)n_a * (int64_t)n_b) return pce_fail(c, PCE_E_INVALID, "pce_seqmatch: all pairs of %d x %d strings are not %lld", n_a, n_b, (long long)n_pairs);
    if (n_pairs && !out_matches) return PCE_E_INVALID;
    PCE_HIP(c, hipSetDevice(c->device));
    SmDevice d;
    PCE_TRY(sm_run(c, "pce_seqmatch", a_chars, a_off, n_a, b_chars, b_off, n_b, pair_a, pair_b, n_pairs, autojunk, d));
    if (n_pairs) PCE_FETCH(c, out_matches, d.out.p, (size_t)n_pairs);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

int pce_seqmatch_align(pce_ctx *c, const uint32_t *a_chars, const int64_t *a_off, int32_t n_a, const uint32_t *b_chars, const int64_t *b_off, int32_t n_b,
                       int32_t autojunk, double *sim, int32_t *match_a, int32_t *match_b, int32_t *n_matches)
{
    const int64_t cells = (int64_t)(n_a > 0 ? n_a : 0) * (int64_t)(n_b > 0 ? n_b : 0);
    PCE_TRY(sm_check_args(c, "pce_seqmatch_align", a_off, n_a, b_off, n_b, cells));
    if (!n_matches || (cells && (!match_a || !match_b))) return PCE_E_INVALID;
    PCE_HIP(c, hipSetDevice(c->device));
    SmDevice d;
    PCE_TRY(sm_run(c, "pce_seqmatch_align", a_chars, a_off, n_a, b_chars, b_off, n_b, nullptr, nullptr, cells, autojunk, d));
    *n_matches = 0;
    if (!cells) { PCE_HIP(c, hipStreamSynchronize(c->stream)); pce_profile_collect(c); return PCE_OK; }
    const size_t tr_ld = ((size_t)n_b + 15) / 16, k_max = (size_t)std::min(n_a, n_b);
    DevBuf dsim, dtr, drows, dma, dmb, dn;
    if (sim) PCE_HIP(c, dsim.reserve(sizeof(double) * (size_t)cells));
    PCE_HIP(c, dtr.reserve(sizeof(unsigned) * (size_t)n_a * tr_ld));
    PCE_HIP(c, drows.reserve(sizeof(double) * (n_a > AL_ROWS ? 2 * ((size_t)n_b + 1) : 1)));
    PCE_HIP(c, dma.reserve(sizeof(int) * k_max)); PCE_HIP(c, dmb.reserve(sizeof(int) * k_max)); PCE_HIP(c, dn.reserve(sizeof(int)));
    int threads = 64; while (threads < n_a && threads < AL_ROWS) threads <<= 1;
    {
        KernelTimer t(c, PCE_K_SEQMATCH_ALIGN, nullptr, (double)cells);
        hipLaunchKernelGGL(k_seqmatch_align, dim3(1), dim3((unsigned)threads), 0, c->stream, d.out.as<int>(), d.ao.as<long long>(), (int)n_a,
                           d.bo.as<long long>(), (int)n_b, sim ? dsim.as<double>() : nullptr, dtr.as<unsigned>(), (long long)tr_ld, drows.as<double>(),
                           dma.as<int>(), dmb.as<int>(), dn.as<int>());
    }
    PCE_HIP(c, hipGetLastError());
    if (sim) PCE_FETCH(c, sim, dsim.p, (size_t)cells);
    PCE_FETCH(c, match_a, dma.p, k_max);
    PCE_FETCH(c, match_b, dmb.p, k_max);
    PCE_FETCH(c, n_matches, dn.p, 1);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

} // extern "C"
