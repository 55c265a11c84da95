// pce_ivl.hip -- the text matching of the aligner evaluation (Code/whisper_testing/splitting.py:94-128, align_intervals) for batches of
// problems: every gold interval, in list order, takes the unclaimed predicted interval of the highest score above 0.4, the first one in
// list order on a tie (the reference replaces its best on a strict > only).  The score of a pair depends on its two normalised texts
// alone -- 1.0 equal, 0.8 one a substring of the other (the empty string is a substring of everything), 0.5 a shared whitespace-separated
// word, else 0 -- so one CLASS TABLE per (gold tier, predicted tier) pair serves the entire-audio call, every 15 s window and every
// sentence of a recording: they differ in the gold rows they walk and in the predicted intervals that are members (include/pce.h).
//
// k_ivl_classes: a wave takes one gold interval and 64 consecutive predicted ones, one per lane, and tests in the reference's order: equal,
// either-is-substring, shared word id (the host interns the words of a call: equal id = equal word).  The three classes leave the wave as
// three 64-bit __ballot masks, exclusive (a pair sets the bit of its first test that holds); row r of a table is [class 3 | 2 | 1] x W
// words, W = ceil(P / 64), bits at and beyond P zero.  Every loop counter is wave-uniform, so every index into the gold interval's code
// points and word ids is, and those reads are scalar loads; the lane's own string is read from global memory.  The nested search ends a
// start as soon as no lane still matches.  No string length limit.
//
// k_ivl_claim: one wave per problem, no barrier.  Subsets keep list order, so "the first unclaimed member of the best class" is the lowest
// set bit of class_row & available, available = member & ~used, class 3 first, then 2, then 1: one key (3 - class, index) per lane, one
// wave minimum (pce_wave.h).  Lane l owns words l, l + 64, ... of `available` -- the first IVL_REG_WORDS of them in registers, the rest in
// LDS -- and only the owner of the winning word reads or writes it: no lane ever reads another lane's word.  The rows of the next gold
// interval do not depend on what was claimed: words 0 .. 64 IVL_REG_WORDS - 1 of them (tiers of up to 8 192 predictions: all of them) are
// loaded one step ahead, and the gold index two steps ahead, so up to that size the sequential chain issues no load it must wait for at
// once; the words of a wider tier are read from global memory inside the step.  A problem's output depends on its own lists and its
// table pair only.
//
// Table pairs run in groups of consecutive pairs whose class tables fit PCE_IVL_TABLE_MB MiB together (read at pce_create).
#include "pce_internal.h"
#include "pce_wave.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int IC_WAVES = 4;              // (gold interval, 64 predicted) tasks in flight per workgroup of k_ivl_classes
constexpr long long IC_MAX_BLOCKS = 1 << 20;     // workgroups of one k_ivl_classes launch: 2^28 work-items, whatever the tables' size
constexpr int IVL_REG_WORDS = 2;         // words of `available` (and of the prefetched rows) a lane of k_ivl_claim keeps in registers
constexpr int IVL_NONE = 0x7fffffff;     // the key of a lane that found nothing
constexpr int IVL_KEY_SHIFT = 20;        // key = (3 - class) << 20 | predicted index; PCE_IVL_MAX_PRED = 2^18 indices
static_assert(PCE_IVL_MAX_PRED <= (1 << IVL_KEY_SHIFT), "a predicted index must fit below the class bits of a key");

struct IvlPair {                         // one table pair of the group in flight
    long long task0;                     // first wave task of k_ivl_classes (tasks: gold row-major, 64-interval chunks inside)
    long long cls0;                      // first word of its class table inside the group's buffer
    int g0, p0;                          // first gold / predicted interval inside the concatenated tiers
    int G, P, W;                         // gold rows, predicted intervals, words per class row
    int pad;
};
struct IvlProblem {
    long long cls0;                      // its pair's class table
    long long list0;                     // first entry of its gold list (and of its outputs)
    long long mem0;                      // first word of its membership bitmap, -1: every predicted interval is a member
    int n, W;
};

__device__ __forceinline__ int wave_min_i32(int v) { return -wave_dpp_max_i32(-v); }        // (v > INT_MIN: lengths, keys)

// one wave task: gold row g of a pair against its predicted intervals 64 ch .. 64 ch + 63 (task: wave-uniform)
__device__ __forceinline__ void ivl_class_task(const unsigned *__restrict__ g_chars, const long long *__restrict__ g_off, const int *__restrict__ g_words,
                                               const long long *__restrict__ g_woff, const unsigned *__restrict__ p_chars,
                                               const long long *__restrict__ p_off, const int *__restrict__ p_words,
                                               const long long *__restrict__ p_woff, const IvlPair *__restrict__ pairs, int n_pairs, long long task,
                                               int lane, unsigned long long *__restrict__ cls)
{
    int lo = 0, hi = n_pairs - 1;                                         // the last pair whose first task is <= task
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (pairs[mid].task0 <= task) lo = mid; else hi = mid - 1; }
    const IvlPair pr = pairs[lo];
    const long long local = task - pr.task0;
    const int g = (int)(local / pr.W), ch = (int)(local % pr.W);
    const long long gi = (long long)pr.g0 + g;
    const long long ga = g_off[gi], gwa = g_woff[gi];
    const int lg = __builtin_amdgcn_readfirstlane((int)(g_off[gi + 1] - ga)), ngw = __builtin_amdgcn_readfirstlane((int)(g_woff[gi + 1] - gwa));
    const unsigned *Gs = g_chars + ga;
    const int *Gw = g_words + gwa;
    const int j = (ch << 6) + lane;
    const bool valid = j < pr.P;
    long long pa = 0, pwa = 0;
    int lp = 0, npw = 0;
    if (valid) {
        const long long pi = (long long)pr.p0 + j;
        pa = p_off[pi]; lp = (int)(p_off[pi + 1] - pa);
        pwa = p_woff[pi]; npw = (int)(p_woff[pi + 1] - pwa);
    }
    const unsigned *Ps = p_chars + pa;
    const int *Pw = p_words + pwa;

    // 1.0: equal
    bool eq = valid && lp == lg;
    for (int k = 0; k < lg && __any(eq); k++) {
        const unsigned gc = Gs[k];
        if (eq && Ps[k] != gc) eq = false;
    }
    // 0.8: one a substring of the other.  Strings of equal length that are not equal hold neither.
    bool sub = false;
    {   // the gold text is the shorter one: is it inside the lane's?
        const bool a = valid && lp > lg;
        if (lg == 0) sub = a;
        else {
            const int max_s = wave_dpp_max_i32(a ? lp - lg : -1);
            for (int s = 0; s <= max_s; s++) {
                if (!__any(a && !sub && s <= lp - lg)) { if (!__any(a && !sub)) break; continue; }
                bool m = a && !sub && s <= lp - lg;
                for (int k = 0; k < lg; k++) {
                    const unsigned gc = Gs[k];
                    if (m && Ps[s + k] != gc) m = false;
                    if (!__any(m)) break;
                }
                sub = sub || m;
            }
        }
    }
    {   // the lane's text is the shorter one: is it inside the gold text?
        const bool b = valid && lp < lg;
        if (b && lp == 0) sub = true;
        const bool b1 = b && lp > 0;
        if (__any(b1)) {
            const int min_lp = wave_min_i32(b1 ? lp : IVL_NONE);
            for (int s = 0; s <= lg - min_lp; s++) {
                bool m = b1 && !sub && s <= lg - lp;
                if (!__any(m)) { if (!__any(b1 && !sub)) break; continue; }
                for (int k = 0;; k++) {                                  // some lane holds m and k < lp here, and for that lane s + k < lg
                    const unsigned gc = Gs[s + k];
                    if (m && k < lp && Ps[k] != gc) m = false;
                    if (!__any(m && k + 1 < lp)) break;
                }
                sub = sub || m;
            }
        }
    }
    // 0.5: a word of the gold text is a word of the lane's
    bool word = false;
    {
        const bool c0 = valid && !eq && !sub && npw > 0;
        if (ngw > 0 && __any(c0)) {
            const int max_w = wave_dpp_max_i32(c0 ? npw : 0);
            for (int x = 0; x < ngw && __any(c0 && !word); x++) {
                const int gw = Gw[x];
                for (int y = 0; y < max_w; y++)
                    if (c0 && y < npw && Pw[y] == gw) word = true;
            }
        }
    }
    const unsigned long long m3 = __ballot(eq), m2 = __ballot(sub && !eq), m1 = __ballot(word && !eq && !sub);
    if (lane == 0) {
        unsigned long long *row = cls + pr.cls0 + (long long)g * 3 * pr.W + ch;
        row[0] = m3; row[pr.W] = m2; row[2 * (long long)pr.W] = m1;
    }
}

// a fixed grid of waves strides over the tasks: the launch's size does not grow with the tables (a dispatch counts its work-items in 32 bits)
__global__ __launch_bounds__(WAVE_SIZE * IC_WAVES) void k_ivl_classes(const unsigned *__restrict__ g_chars, const long long *__restrict__ g_off,
                                                                     const int *__restrict__ g_words, const long long *__restrict__ g_woff,
                                                                     const unsigned *__restrict__ p_chars, const long long *__restrict__ p_off,
                                                                     const int *__restrict__ p_words, const long long *__restrict__ p_woff,
                                                                     const IvlPair *__restrict__ pairs, int n_pairs, long long n_tasks,
                                                                     unsigned long long *__restrict__ cls)
{
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long n_waves = (long long)gridDim.x * IC_WAVES;
    for (long long task = (long long)blockIdx.x * IC_WAVES + w; task < n_tasks; task += n_waves)      // (wave-uniform)
        ivl_class_task(g_chars, g_off, g_words, g_woff, p_chars, p_off, p_words, p_woff, pairs, n_pairs, task, lane, cls);
}

__global__ __launch_bounds__(WAVE_SIZE) void k_ivl_claim(const unsigned long long *__restrict__ cls, const IvlProblem *__restrict__ problems,
                                                         const int *__restrict__ ids, const int *__restrict__ gold_idx,
                                                         const unsigned long long *__restrict__ member, int *__restrict__ out_match,
                                                         signed char *__restrict__ out_class)
{
    extern __shared__ unsigned long long avail_lds[];                    // words IVL_REG_WORDS * 64 .. W of `available`
    const int lane = threadIdx.x;
    const IvlProblem pb = problems[ids[blockIdx.x]];
    const int n = pb.n, W = pb.W;
    const unsigned long long *mem = pb.mem0 >= 0 ? member + pb.mem0 : nullptr;
    const int *list = gold_idx + pb.list0;
    unsigned long long av[IVL_REG_WORDS];
#pragma unroll
    for (int k = 0; k < IVL_REG_WORDS; k++) {
        const int x = lane + 64 * k;
        av[k] = x < W ? (mem ? mem[x] : ~0ull) : 0ull;
    }
    for (int x = lane + 64 * IVL_REG_WORDS; x < W; x += 64) avail_lds[x - 64 * IVL_REG_WORDS] = mem ? mem[x] : ~0ull;
    // rows one step ahead, gold indices two
    unsigned long long nxt[3][IVL_REG_WORDS];
    int g_next = n > 0 ? list[0] : 0, g_after = n > 1 ? list[1] : 0;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < IVL_REG_WORDS; k++) {
            const int x = lane + 64 * k;
            nxt[c][k] = (n > 0 && x < W) ? cls[pb.cls0 + ((long long)g_next * 3 + c) * W + x] : 0ull;
        }
    for (int i = 0; i < n; i++) {
        unsigned long long cur[3][IVL_REG_WORDS];
        const unsigned long long *row = cls + pb.cls0 + (long long)g_next * 3 * W;
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int k = 0; k < IVL_REG_WORDS; k++) cur[c][k] = nxt[c][k];
        g_next = g_after;
        if (i + 1 < n) {
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int k = 0; k < IVL_REG_WORDS; k++) {
                    const int x = lane + 64 * k;
                    nxt[c][k] = x < W ? cls[pb.cls0 + ((long long)g_next * 3 + c) * W + x] : 0ull;
                }
        }
        g_after = i + 2 < n ? list[i + 2] : 0;
        int key = IVL_NONE;
#pragma unroll
        for (int c = 0; c < 3; c++) {                                    // c = 0: class 3 (equal) .. c = 2: class 1 (shared word)
#pragma unroll
            for (int k = 0; k < IVL_REG_WORDS; k++) {
                const unsigned long long x = cur[c][k] & av[k];
                if (x) key = min(key, (c << IVL_KEY_SHIFT) | ((lane + 64 * k) << 6) | (int)__builtin_ctzll(x));
            }
            // a lane's words ascend: its first hit of a class is its lowest, and a lane that holds a hit of a better class needs none
            for (int xw = lane + 64 * IVL_REG_WORDS; xw < W && (key >> IVL_KEY_SHIFT) > c; xw += 64) {
                const unsigned long long x = row[(long long)c * W + xw] & avail_lds[xw - 64 * IVL_REG_WORDS];
                if (x) { key = min(key, (c << IVL_KEY_SHIFT) | (xw << 6) | (int)__builtin_ctzll(x)); break; }
            }
        }
        const int best = wave_min_i32(key);                              // wave-uniform
        int match = -1, klass = 0;
        if (best != IVL_NONE) {
            match = best & ((1 << IVL_KEY_SHIFT) - 1); klass = 3 - (best >> IVL_KEY_SHIFT);
            const int xw = match >> 6;
            const unsigned long long bit = 1ull << (match & 63);
            if ((xw & 63) == lane) {                                     // the word's owner marks it claimed
#pragma unroll
                for (int k = 0; k < IVL_REG_WORDS; k++) if ((xw >> 6) == k) av[k] &= ~bit;
                if ((xw >> 6) >= IVL_REG_WORDS) avail_lds[xw - 64 * IVL_REG_WORDS] &= ~bit;
            }
        }
        if (lane == 0) { out_match[pb.list0 + i] = match; out_class[pb.list0 + i] = (signed char)klass; }
    }
}

// offsets [n + 1] of a concatenated table: from 0, not decreasing; elements present when the offsets say so
int ivl_check_offsets(pce_ctx *c, const char *which, const void *elems, const int64_t *off, int32_t n)
{
    if (off[0] != 0) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: %s offsets must start at 0", which);
    for (int32_t s = 0; s < n; s++)
        if (off[s + 1] < off[s]) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: %s offsets decrease at interval %d", which, s);
    if (off[n] && !elems) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: %s table has offsets but no elements", which);
    for (int32_t s = 0; s < n; s++)
        if (off[s + 1] - off[s] > 0x3fffffff) return pce_fail(c, PCE_E_LIMIT, "pce_ivl_match: %s interval %d has 2^30 elements or more", which, s);
    return PCE_OK;
}

int ivl_check_ranges(pce_ctx *c, const char *which, const int32_t *range, int32_t n_pairs, int32_t n)
{
    if (range[0] != 0) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: the %s ranges must start at 0", which);
    for (int32_t t = 0; t < n_pairs; t++)
        if (range[t + 1] < range[t]) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: the %s ranges decrease at pair %d", which, t);
    if (range[n_pairs] != n) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: the %s ranges end at %d of %d intervals", which, range[n_pairs], n);
    return PCE_OK;
}

} // namespace

extern "C" {

int pce_ivl_match(pce_ctx *c, const uint32_t *g_chars, const int64_t *g_off, const int32_t *g_words, const int64_t *g_woff, int32_t n_gold,
                  const uint32_t *p_chars, const int64_t *p_off, const int32_t *p_words, const int64_t *p_woff, int32_t n_pred,
                  const int32_t *pair_gold, const int32_t *pair_pred, int32_t n_pairs, const int32_t *prob_pair, const int64_t *prob_off,
                  const int32_t *gold_idx, const int64_t *member_off, const uint64_t *member, int32_t n_problems, int32_t *out_match,
                  int8_t *out_class)
{
    if (!c) return PCE_E_INVALID;
    if (n_gold < 0 || n_pred < 0 || n_pairs < 0 || n_problems < 0) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: a negative count");
    if (!g_off || !g_woff || !p_off || !p_woff || !pair_gold || !pair_pred) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: null offsets or ranges");
    if (n_problems && (!prob_pair || !prob_off)) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: problems without their pair indices or offsets");
    PCE_TRY(ivl_check_offsets(c, "gold text", g_chars, g_off, n_gold));
    PCE_TRY(ivl_check_offsets(c, "gold word", g_words, g_woff, n_gold));
    PCE_TRY(ivl_check_offsets(c, "predicted text", p_chars, p_off, n_pred));
    PCE_TRY(ivl_check_offsets(c, "predicted word", p_words, p_woff, n_pred));
    PCE_TRY(ivl_check_ranges(c, "gold", pair_gold, n_pairs, n_gold));
    PCE_TRY(ivl_check_ranges(c, "predicted", pair_pred, n_pairs, n_pred));
    if (n_problems == 0) return PCE_OK;
    // the problems: their pair, their gold rows, their bitmap
    if (prob_off[0] != 0) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: the problem offsets must start at 0");
    std::vector<int64_t> mem_words((size_t)n_pairs, 0);                  // W of every pair
    for (int32_t t = 0; t < n_pairs; t++) {
        const int64_t P = (int64_t)pair_pred[t + 1] - pair_pred[t];
        if (P > PCE_IVL_MAX_PRED) return pce_fail(c, PCE_E_LIMIT, "pce_ivl_match: pair %d has %lld predicted intervals, at most %d", t, (long long)P, (int)PCE_IVL_MAX_PRED);
        mem_words[(size_t)t] = div_up(P, 64);
    }
    int64_t member_end = 0;
    std::vector<char> pair_used((size_t)n_pairs, 0);
    for (int32_t q = 0; q < n_problems; q++) {
        const int64_t len = prob_off[q + 1] - prob_off[q];
        if (len < 0) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: the problem offsets decrease at problem %d", q);
        if (len > 0x7fffffff) return pce_fail(c, PCE_E_LIMIT, "pce_ivl_match: problem %d lists 2^31 gold intervals or more", q);
        const int32_t t = prob_pair[q];
        if (t < 0 || t >= n_pairs) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: problem %d names pair %d of %d", q, t, n_pairs);
        if (len && !gold_idx) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: gold lists without their indices");
        const int32_t G = pair_gold[t + 1] - pair_gold[t];
        for (int64_t x = prob_off[q]; x < prob_off[q + 1]; x++)
            if (gold_idx[x] < 0 || gold_idx[x] >= G) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: problem %d lists gold interval %d of a tier of %d", q, gold_idx[x], G);
        if (member_off && member_off[q] >= 0) {
            if (!member && mem_words[(size_t)t]) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: problem %d has a bitmap offset but there are no bitmaps", q);
            if (mem_words[(size_t)t]) member_end = std::max(member_end, member_off[q] + mem_words[(size_t)t]);
        }
        if (len) pair_used[(size_t)t] = 1;
    }
    const int64_t n_slots = prob_off[n_problems];
    if (n_slots == 0) return PCE_OK;
    if (!out_match || !out_class) return pce_fail(c, PCE_E_INVALID, "pce_ivl_match: null outputs");
    // groups of consecutive pairs whose class tables fit the budget (a pair no problem walks takes no room)
    std::vector<int64_t> words((size_t)n_pairs, -1);
    for (int32_t t = 0; t < n_pairs; t++)
        if (pair_used[(size_t)t]) words[(size_t)t] = (int64_t)(pair_gold[t + 1] - pair_gold[t]) * 3 * mem_words[(size_t)t];
    const SweepGroups groups = sweep_groups(words, (int64_t)(c->sw.ivl_table_budget / 8));
    if (groups.too_large >= 0) {
        const size_t t = (size_t)groups.too_large;
        return pce_fail(c, PCE_E_LIMIT, "pce_ivl_match: pair %zu (%d gold, %d predicted intervals) needs %.1f MiB of class tables, the budget is %.1f MiB (PCE_IVL_TABLE_MB)", t,
                        pair_gold[t + 1] - pair_gold[t], pair_pred[t + 1] - pair_pred[t], words[t] * 8.0 / 1048576.0, c->sw.ivl_table_budget / 1048576.0);
    }
    PCE_HIP(c, hipSetDevice(c->device));
    struct { DevBuf gc, go, gw, gwo, pc, po, pw, pwo, pairs, probs, ids, list, mem, cls, match, klass; } d;
    PCE_UPLOAD(c, d.gc, g_chars, (size_t)g_off[n_gold], 1); PCE_UPLOAD(c, d.go, g_off, (size_t)n_gold + 1);
    PCE_UPLOAD(c, d.gw, g_words, (size_t)g_woff[n_gold], 1); PCE_UPLOAD(c, d.gwo, g_woff, (size_t)n_gold + 1);
    PCE_UPLOAD(c, d.pc, p_chars, (size_t)p_off[n_pred], 1); PCE_UPLOAD(c, d.po, p_off, (size_t)n_pred + 1);
    PCE_UPLOAD(c, d.pw, p_words, (size_t)p_woff[n_pred], 1); PCE_UPLOAD(c, d.pwo, p_woff, (size_t)n_pred + 1);
    PCE_UPLOAD(c, d.list, gold_idx, (size_t)n_slots);
    PCE_UPLOAD(c, d.mem, member, (size_t)member_end, 1);
    PCE_HIP(c, d.cls.reserve(sizeof(unsigned long long) * (size_t)std::max<int64_t>(groups.largest, 1)));
    PCE_HIP(c, d.match.reserve(sizeof(int) * (size_t)n_slots)); PCE_HIP(c, d.klass.reserve((size_t)n_slots));
    // per group: its pairs' tables, then the problems that walk them
    std::vector<IvlPair> tab((size_t)n_pairs);
    std::vector<IvlProblem> probs((size_t)n_problems);
    std::vector<int> ids;
    std::vector<size_t> group_of((size_t)n_pairs, 0), first_id;
    {
        size_t t0 = 0;
        for (size_t gr = 0; gr < groups.group_end.size(); gr++) { for (size_t t = t0; t < groups.group_end[gr]; t++) group_of[t] = gr; t0 = groups.group_end[gr]; }
    }
    for (int32_t t = 0; t < n_pairs; t++)
        tab[(size_t)t] = {0, groups.offset[(size_t)t], pair_gold[t], pair_pred[t], pair_gold[t + 1] - pair_gold[t], pair_pred[t + 1] - pair_pred[t],
                          (int)mem_words[(size_t)t], 0};
    for (int32_t q = 0; q < n_problems; q++) {
        const size_t t = (size_t)prob_pair[q];
        probs[(size_t)q] = {tab[t].cls0, prob_off[q], (member_off && member_off[q] >= 0) ? member_off[q] : -1, (int)(prob_off[q + 1] - prob_off[q]), tab[t].W};
    }
    for (size_t gr = 0; gr < groups.group_end.size(); gr++) {            // the ids of every group's problems, empty lists left out
        first_id.push_back(ids.size());
        for (int32_t q = 0; q < n_problems; q++)
            if (probs[(size_t)q].n > 0 && group_of[(size_t)prob_pair[q]] == gr) ids.push_back(q);
    }
    first_id.push_back(ids.size());
    PCE_UPLOAD(c, d.probs, probs); PCE_UPLOAD(c, d.ids, ids);
    PCE_HIP(c, d.pairs.reserve(sizeof(IvlPair) * (size_t)n_pairs));
    std::vector<std::vector<IvlPair>> group_pairs(groups.group_end.size());     // (they live until the stream has taken them)
    size_t t0 = 0;
    for (size_t gr = 0; gr < groups.group_end.size(); gr++) {
        const size_t te = groups.group_end[gr];
        std::vector<IvlPair> &gp = group_pairs[gr];
        long long n_tasks = 0;
        double tested = 0.0, steps = 0.0;
        int max_W = 0;
        for (size_t t = t0; t < te; t++) {
            if (!pair_used[t] || tab[t].G == 0 || tab[t].W == 0) continue;
            IvlPair p = tab[t]; p.task0 = n_tasks; gp.push_back(p);
            n_tasks += (long long)p.G * p.W; tested += (double)p.G * (double)p.P;
            max_W = std::max(max_W, p.W);
        }
        const size_t n_ids = first_id[gr + 1] - first_id[gr];
        for (size_t x = first_id[gr]; x < first_id[gr + 1]; x++) steps += (double)probs[(size_t)ids[x]].n;
        for (size_t t = t0; t < te; t++) if (pair_used[t]) max_W = std::max(max_W, tab[t].W);
        t0 = te;
        if (n_tasks > 0) {
            PCE_PUT(c, d.pairs.p, gp.data(), gp.size());
            KernelTimer tm(c, PCE_K_IVL_CLASSES, nullptr, tested);
            hipLaunchKernelGGL(k_ivl_classes, dim3((unsigned)std::min<long long>(div_up(n_tasks, IC_WAVES), IC_MAX_BLOCKS)), dim3(WAVE_SIZE * IC_WAVES), 0, c->stream, d.gc.as<unsigned>(),
                               d.go.as<long long>(), d.gw.as<int>(), d.gwo.as<long long>(), d.pc.as<unsigned>(), d.po.as<long long>(), d.pw.as<int>(),
                               d.pwo.as<long long>(), d.pairs.as<IvlPair>(), (int)gp.size(), n_tasks, d.cls.as<unsigned long long>());
        }
        PCE_HIP(c, hipGetLastError());
        if (n_ids > 0) {
            const size_t lds = sizeof(unsigned long long) * (size_t)std::max(max_W - 64 * IVL_REG_WORDS, 0);
            KernelTimer tm(c, PCE_K_IVL_CLAIM, nullptr, steps);
            hipLaunchKernelGGL(k_ivl_claim, dim3((unsigned)n_ids), dim3(WAVE_SIZE), lds, c->stream, d.cls.as<unsigned long long>(), d.probs.as<IvlProblem>(),
                               d.ids.as<int>() + first_id[gr], d.list.as<int>(), d.mem.as<unsigned long long>(), d.match.as<int>(), d.klass.as<signed char>());
        }
        PCE_HIP(c, hipGetLastError());
    }
    PCE_FETCH(c, out_match, d.match.p, (size_t)n_slots);
    PCE_FETCH(c, out_class, d.klass.p, (size_t)n_slots);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    return PCE_OK;
}

} // extern "C"
