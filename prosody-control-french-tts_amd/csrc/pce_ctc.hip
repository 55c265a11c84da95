// pce_ctc.hip -- CTC forced alignment: the Viterbi pass over the 2 L + 1 blank-interleaved states of a transcript, for a batch of clips.
//
// One of the reference's aligners (Code/Aligners/CTCFA.py through the ctc-forced-aligner command) rests on this dynamic programme;
// Code/Aligners/whisperX.py does not: it runs its own trellis and back-track (pce_wx.hip).  The recurrence is the CPU implementation of torchaudio.functional.forced_align; that
// package is third party and absent: restated from its published source, parity unpinned.  State i carries `blank` (i even) or
// targets[i / 2] (i odd).  alpha_0[0] = lp[0][blank], alpha_0[1] = lp[0][targets[0]], the rest -inf.  For t >= 1:
//     x0 = alpha[i],  x1 = alpha[i - 1],  x2 = alpha[i - 2] where i is odd, i != 1 and targets[i / 2] != targets[i / 2 - 1], else -inf
//     x2 > x1 && x2 > x0: x2, back-pointer 2;  else x1 > x0 && x1 > x2: x1, back-pointer 1;  else x0, back-pointer 0   (x1 == x2 > x0 takes x0)
//     alpha'[i] = fp32(chosen + lp[t][label(i)])
// the final state is 2 L if alpha[2 L] > alpha[2 L - 1], else 2 L - 1.  fp32 adds and compares only (no FMA can form: there is no multiply): a
// CPU restatement of these lines is bit-identical.  torchaudio's moving start / end window only leaves out states no complete path can visit;
// it is not restated (every state is computed: the outputs are the same).
//
// k_ctc<false / true>  REGISTER FORM.  A thread owns CTC_RUN consecutive states in registers.  CTC_RUN is even, so a thread's first state is a
//     blank: it needs alpha[i - 1] only, and the thread's second state takes the same value as its alpha[i - 2].  That value is the last state
//     of the thread before it: ONE DPP wave shift per frame (the idiom of k_levenshtein, pce_align.hip).  <false>: a clip whose states fit
//     one wave runs on one wave, no LDS and no barrier, four clips per workgroup.  <true>: one workgroup per clip; the top state of a wave
//     crosses to lane 0 of the next through an LDS slot, double buffered by frame parity: ONE barrier per frame.  The emission of a state
//     depends on t only: frame t + 1's values are loaded while frame t is computed, so no load sits on the DATA dependency chain.  The
//     prefetch is one frame deep and is waited for at the end of frame t (in <true>, by the barrier's own wait, which also drains the trace
//     store): a frame costs at least max(its arithmetic, one load latency).  Up to CTC_REG_STATES states.
// k_ctc_general        GENERAL FORM, any L: one workgroup per clip, the two alpha rows in HBM scratch, threads loop over chunks of states.  Slow, correct.
// k_ctc_trace          one wave per clip, lane 0 walks the back-pointers from the final state to t = 0 and writes path, frame_score, tok_first,
//     tok_last, score and status.
//
// Trace: 2 bits per state, the CTC_RUN states of a thread in one byte, four frames of a thread in one 32-bit word: word (t / 4) * NT + thread
// (NT = threads that sweep the clip), so a wave stores 256 contiguous bytes every fourth frame.  The general form writes the same layout by bytes.
// Clips run in groups whose traces fit PCE_CTC_TRACE_MB MiB (read at pce_create); a clip's outputs depend on its own emissions and targets only.
#include "pce_internal.h"
#include "pce_wave.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int CTC_RUN = 4;                                  // states per thread (one trace byte)
static_assert(CTC_RUN % 2 == 0 && CTC_RUN >= 2, "a thread's first state must be a blank: only then does one value cross between threads");
constexpr int CTC_MAX_THREADS = 1024;
constexpr int CTC_REG_STATES = PCE_CTC_REG_STATES;          // the register form's limit
static_assert(CTC_REG_STATES == CTC_RUN * CTC_MAX_THREADS, "include/pce.h states the register form's limit");
constexpr int CTC_GEN_THREADS = 256;

struct CtcClip {
    long long row0;      // first emission row
    long long tgt0;      // first target (and first tok_first / tok_last entry)
    long long trace0;    // first trace word inside the group's trace
    long long out0;      // first entry of path / frame_score
    long long scr0;      // general form: first float of its two alpha rows
    int T, L, NT, pad;   // NT: threads (register form) or groups of CTC_RUN states (general form) per frame of trace
};

__device__ __forceinline__ void ctc_choose(float x0, float x1, float x2, float &chosen, unsigned &bp)
{
    if (x2 > x1 && x2 > x0) { chosen = x2; bp = 2u; }
    else if (x1 > x0 && x1 > x2) { chosen = x1; bp = 1u; }
    else { chosen = x0; bp = 0u; }
}

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? CTC_MAX_THREADS : 256) PCE_NO_PK_F32 void k_ctc(const float *__restrict__ lp, int V, int blank, const int *__restrict__ targets,
                                                                                     const CtcClip *__restrict__ clips, const int *__restrict__ ids, int n_ids,
                                                                                     unsigned *__restrict__ trace, float *__restrict__ fin)
{
    __shared__ float xch[2][CTC_MAX_THREADS / WAVE_SIZE];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int slot = MULTI ? (int)blockIdx.x : (int)blockIdx.x * 4 + wave;
    if (slot >= n_ids) return;                               // (<false> only: a whole wave leaves, and that form has no barrier)
    const int c = ids[slot];
    const CtcClip cl = clips[c];
    const int S = 2 * cl.L + 1, T = cl.T, NT = cl.NT;
    const int tid = MULTI ? (int)threadIdx.x : lane;
    const int *tg = targets + cl.tgt0;
    const float NINF = -INFINITY;

    int lab[CTC_RUN];
    bool live[CTC_RUN], skip[CTC_RUN];
#pragma unroll
    for (int k = 0; k < CTC_RUN; k++) {
        const int i = tid * CTC_RUN + k;
        live[k] = i < S;
        const bool odd = live[k] && (i & 1);
        const int own = odd ? tg[i >> 1] : blank;
        lab[k] = own;
        skip[k] = odd && i >= 3 && own != tg[(i >> 1) - 1];
    }
    const float *row = lp + cl.row0 * (long long)V;
    float a[CTC_RUN], e[CTC_RUN], en[CTC_RUN];
#pragma unroll
    for (int k = 0; k < CTC_RUN; k++) {
        const int i = tid * CTC_RUN + k;
        a[k] = (live[k] && i < 2) ? row[lab[k]] : NINF;
        en[k] = 0.0f;
    }
    row += V;
    if (T > 1) {
#pragma unroll
        for (int k = 0; k < CTC_RUN; k++) e[k] = row[lab[k]];
    } else {
#pragma unroll
        for (int k = 0; k < CTC_RUN; k++) e[k] = 0.0f;
    }
    if (MULTI) {
        if (lane == 63) xch[0][wave] = a[CTC_RUN - 1];
        __syncthreads();
    }
    unsigned word = 0u;
    for (int t = 1; t < T; t++) {
        row += V;
        if (t + 1 < T) {                                     // frame t + 1's emissions: in flight while frame t is computed
#pragma unroll
            for (int k = 0; k < CTC_RUN; k++) en[k] = row[lab[k]];
        }
        float p1 = dpp<0x138>(a[CTC_RUN - 1]);               // wave_shr:1 -- alpha[i0 - 1]: the last state of the thread before
        if (lane == 0) p1 = (MULTI && wave > 0) ? xch[(t - 1) & 1][wave - 1] : NINF;
        float na[CTC_RUN];
        unsigned byte = 0u;
#pragma unroll
        for (int k = 0; k < CTC_RUN; k++) {
            const float x0 = a[k], x1 = k >= 1 ? a[k - 1] : p1;
            const float x2 = (k >= 1 && skip[k]) ? (k >= 2 ? a[k - 2] : p1) : NINF;          // (k = 0 is a blank: skip[0] is never set)
            float chosen; unsigned bp;
            ctc_choose(x0, x1, x2, chosen, bp);
            na[k] = live[k] ? chosen + e[k] : NINF;
            byte |= bp << (2 * k);
        }
#pragma unroll
        for (int k = 0; k < CTC_RUN; k++) { a[k] = na[k]; e[k] = en[k]; }
        if (MULTI) {
            if (lane == 63) xch[t & 1][wave] = a[CTC_RUN - 1];
            __syncthreads();
        }
        word |= byte << (8 * (t & 3));
        if ((t & 3) == 3 || t == T - 1) {
            if (tid < NT) trace[cl.trace0 + (long long)(t >> 2) * NT + tid] = word;
            word = 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < CTC_RUN; k++) {
        const int i = tid * CTC_RUN + k;
        if (i == S - 1) fin[2 * c + 1] = a[k];
        if (i == S - 2) fin[2 * c] = a[k];
    }
}

__global__ __launch_bounds__(CTC_GEN_THREADS) PCE_NO_PK_F32 void k_ctc_general(const float *__restrict__ lp, int V, int blank, const int *__restrict__ targets,
                                                                               const CtcClip *__restrict__ clips, const int *__restrict__ ids,
                                                                               unsigned char *__restrict__ trace, float *__restrict__ scratch, float *__restrict__ fin)
{
    const int c = ids[blockIdx.x];
    const CtcClip cl = clips[c];
    const int S = 2 * cl.L + 1, T = cl.T, NT = cl.NT;
    const int *tg = targets + cl.tgt0;
    const float NINF = -INFINITY;
    float *A = scratch + cl.scr0, *B = A + S;
    const float *row = lp + cl.row0 * (long long)V;
    for (int i = threadIdx.x; i < S; i += CTC_GEN_THREADS) A[i] = i < 2 ? row[(i & 1) ? tg[0] : blank] : NINF;
    __syncthreads();
    for (int t = 1; t < T; t++) {
        row += V;
        for (int g = threadIdx.x; g < NT; g += CTC_GEN_THREADS) {
            unsigned byte = 0u;
            for (int k = 0; k < CTC_RUN; k++) {
                const int i = g * CTC_RUN + k;
                if (i >= S) break;
                const int own = (i & 1) ? tg[i >> 1] : blank;
                const bool skip = (i & 1) && i >= 3 && own != tg[(i >> 1) - 1];
                const float x0 = A[i], x1 = i >= 1 ? A[i - 1] : NINF, x2 = skip ? A[i - 2] : NINF;
                float chosen; unsigned bp;
                ctc_choose(x0, x1, x2, chosen, bp);
                B[i] = chosen + row[own];
                byte |= bp << (2 * k);
            }
            trace[(cl.trace0 + (long long)(t >> 2) * NT + g) * 4 + (t & 3)] = (unsigned char)byte;
        }
        __syncthreads();                                     // (workgroup-scope release / acquire of the row just written)
        float *x = A; A = B; B = x;
    }
    if (threadIdx.x == 0) { fin[2 * c + 1] = A[S - 1]; fin[2 * c] = A[S - 2]; }
}

__global__ __launch_bounds__(WAVE_SIZE) void k_ctc_trace(const float *__restrict__ lp, int V, int blank, const int *__restrict__ targets,
                                                         const CtcClip *__restrict__ clips, const int *__restrict__ ids, const unsigned char *__restrict__ trace,
                                                         const float *__restrict__ fin, int *__restrict__ path, float *__restrict__ frame_score,
                                                         int *__restrict__ tok_first, int *__restrict__ tok_last, float *__restrict__ score, int *__restrict__ status)
{
    if (threadIdx.x != 0) return;
    const int c = ids[blockIdx.x];
    const CtcClip cl = clips[c];
    const int T = cl.T, NT = cl.NT;
    const int *tg = targets + cl.tgt0;
    const float f0 = fin[2 * c], f1 = fin[2 * c + 1];
    int i = f1 > f0 ? 2 * cl.L : 2 * cl.L - 1;
    const float sc = f1 > f0 ? f1 : f0;
    score[c] = sc;
    if (sc == -INFINITY || sc != sc) { status[c] = PCE_CTC_NO_PATH; return; }
    status[c] = PCE_CTC_OK;
    int later = -1;                                          // the state of frame t + 1
    for (int t = T - 1; t >= 0; t--) {
        const int own = (i & 1) ? tg[i >> 1] : blank;
        if (path) path[cl.out0 + t] = own;
        if (frame_score) frame_score[cl.out0 + t] = lp[(cl.row0 + t) * (long long)V + own];
        int before = i;
        if (t > 0) {
            const unsigned byte = trace[(cl.trace0 + (long long)(t >> 2) * NT + (i >> 2)) * 4 + (t & 3)];
            before = i - (int)((byte >> (2 * (i & 3))) & 3u);       // (state 0 only ever stays, state 1 never takes alpha[i - 2]: before >= 0)
        }
        if (i & 1) {
            if (i != later) tok_last[cl.tgt0 + (i >> 1)] = t;
            if (t == 0 || before != i) tok_first[cl.tgt0 + (i >> 1)] = t;
        }
        later = i; i = before;
    }
}

} // namespace

extern "C" {

int pce_ctc_align(pce_ctx *c, const float *emissions, int32_t emissions_on_device, const int64_t *row_start, const int32_t *n_frames, int32_t n_vocab,
                  const int32_t *targets, const int64_t *target_off, int32_t n_clips, const pce_ctc_params *p, int32_t *path, float *frame_score,
                  int32_t *tok_first, int32_t *tok_last, float *score, int32_t *status)
{
    if (!c) return PCE_E_INVALID;
    if (!row_start || !n_frames || !target_off || !p || !score || !status || n_clips <= 0 || n_vocab <= 0)
        return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: NULL argument, no clips or no vocabulary");
    if (p->blank < 0 || p->blank >= n_vocab) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: blank %d outside the vocabulary of %d", p->blank, n_vocab);
    if (p->form < 0 || p->form > 2) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: form %d (0 auto, 1 register, 2 general)", p->form);
    if (target_off[0] != 0) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: target offsets must start at 0");
    const size_t n = (size_t)n_clips;
    int64_t row_lo = INT64_MAX, row_hi = 0, total_frames = 0;
    std::vector<CtcClip> tab(n);
    std::vector<int> kind(n, -1);                            // -1: not run; 0: one wave; 1..4: 128 / 256 / 512 / 1024 threads; 5: general form
    for (size_t q = 0; q < n; q++) {
        const int64_t L = target_off[q + 1] - target_off[q], T = n_frames[q];
        if (L < 0 || T < 0 || row_start[q] < 0) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: clip %zu has a negative length or row", q);
        if (L > 0x3fffffff) return pce_fail(c, PCE_E_LIMIT, "pce_ctc_align: clip %zu has more than 2^30 targets", q);
        if (L && !targets) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: targets is NULL");
        int64_t R = 0;
        for (int64_t l = 0; l < L; l++) {
            const int32_t id = targets[target_off[q] + l];
            if (id < 0 || id >= n_vocab || id == p->blank)
                return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: target %lld of clip %zu is %d (vocabulary %d, blank %d)", (long long)l, q, id, n_vocab, p->blank);
            if (l && id == targets[target_off[q] + l - 1]) R++;
        }
        CtcClip &cl = tab[q];
        cl.row0 = row_start[q]; cl.tgt0 = target_off[q]; cl.trace0 = 0; cl.out0 = total_frames; cl.scr0 = 0;
        cl.T = (int)T; cl.L = (int)L; cl.NT = 0; cl.pad = 0;
        total_frames += T;
        status[q] = (L == 0 || T == 0) ? PCE_CTC_EMPTY : (T < L + R ? PCE_CTC_TOO_SHORT : PCE_CTC_OK);
        if (T) { row_lo = std::min<int64_t>(row_lo, row_start[q]); row_hi = std::max<int64_t>(row_hi, row_start[q] + T); }
        if (status[q] != PCE_CTC_OK) continue;
        const int64_t S = 2 * L + 1;
        if (p->form == 1 && S > CTC_REG_STATES)
            return pce_fail(c, PCE_E_LIMIT, "pce_ctc_align: clip %zu has %lld states, the register form holds %d", q, (long long)S, CTC_REG_STATES);
        if (p->form == 2 || S > CTC_REG_STATES) { kind[q] = 5; cl.NT = (int)div_up(S, CTC_RUN); }
        else {
            const int64_t threads = div_up(S, CTC_RUN);
            int k = 0, nt = WAVE_SIZE;
            while (nt < threads) { nt <<= 1; k++; }
            kind[q] = k; cl.NT = nt;
        }
    }
    if ((total_frames && !emissions) || (target_off[n] && (!tok_first || !tok_last))) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: NULL emissions or token outputs");

    // groups of consecutive clips whose traces fit the budget
    const int64_t budget_words = (int64_t)(c->sw.ctc_trace_budget / 4);
    std::vector<size_t> group_end;
    int64_t scratch_floats = 0, max_group_words = 0;
    {
        int64_t words = 0;
        for (size_t q = 0; q < n; q++) {
            if (kind[q] < 0) continue;
            const int64_t w = div_up(tab[q].T, 4) * (int64_t)tab[q].NT;
            if (w > budget_words)
                return pce_fail(c, PCE_E_LIMIT, "pce_ctc_align: clip %zu (%d frames, %d targets) needs %.1f MiB of trace, the budget is %.1f MiB (PCE_CTC_TRACE_MB)", q,
                                tab[q].T, tab[q].L, w * 4.0 / 1048576.0, c->sw.ctc_trace_budget / 1048576.0);
            if (words + w > budget_words) { group_end.push_back(q); words = 0; }
            tab[q].trace0 = words;
            words += w;
            max_group_words = std::max(max_group_words, words);
            if (kind[q] == 5) { tab[q].scr0 = scratch_floats; scratch_floats += 2 * (2 * (int64_t)tab[q].L + 1); }
        }
        group_end.push_back(n);
    }

    PCE_HIP(c, hipSetDevice(c->device));
    auto &d = c->ctc;
    const size_t n_tok = (size_t)target_off[n], nf = (size_t)total_frames;
    const float *d_lp = emissions;
    int64_t row_shift = 0;
    if (!emissions_on_device && nf) {
        PCE_UPLOAD(c, d.lp, emissions + row_lo * (int64_t)n_vocab, (size_t)(row_hi - row_lo) * (size_t)n_vocab);
        d_lp = d.lp.as<float>(); row_shift = row_lo;
    }
    for (size_t q = 0; q < n; q++) tab[q].row0 -= row_shift;
    // id lists: per group, per kind
    std::vector<int> ids; ids.reserve(n);
    struct Launch { int kind; size_t first, count; };
    std::vector<Launch> launches;                            // kind 6: the trace walk of a group
    {
        size_t g0 = 0;
        for (size_t ge : group_end) {
            const size_t first_of_group = ids.size();
            for (int k = 0; k <= 5; k++) {
                const size_t first = ids.size();
                for (size_t q = g0; q < ge; q++) if (kind[q] == k) ids.push_back((int)q);
                if (ids.size() > first) launches.push_back({k, first, ids.size() - first});
            }
            if (ids.size() > first_of_group) launches.push_back({6, first_of_group, ids.size() - first_of_group});
            g0 = ge;
        }
    }
    PCE_HIP(c, d.fin.reserve(sizeof(float) * 2 * n));
    PCE_HIP(c, d.trace.reserve(sizeof(unsigned) * (size_t)(max_group_words + 1))); PCE_HIP(c, d.scratch.reserve(sizeof(float) * (size_t)(scratch_floats + 1)));
    PCE_HIP(c, d.path.reserve(sizeof(int) * (nf + 1))); PCE_HIP(c, d.fscore.reserve(sizeof(float) * (nf + 1)));
    PCE_HIP(c, d.first.reserve(sizeof(int) * (n_tok + 1))); PCE_HIP(c, d.last.reserve(sizeof(int) * (n_tok + 1)));
    PCE_HIP(c, d.score.reserve(sizeof(float) * n));
    PCE_UPLOAD(c, d.tab, tab); PCE_UPLOAD(c, d.ids, ids, 1); PCE_UPLOAD(c, d.tgt, targets, n_tok, 1); PCE_UPLOAD(c, d.status, status, (size_t)n);
    if (n_tok) { PCE_HIP(c, hipMemsetAsync(d.first.p, 0xFF, sizeof(int) * n_tok, c->stream)); PCE_HIP(c, hipMemsetAsync(d.last.p, 0xFF, sizeof(int) * n_tok, c->stream)); }
    if (nf) { PCE_HIP(c, hipMemsetAsync(d.path.p, 0xFF, sizeof(int) * nf, c->stream)); PCE_HIP(c, hipMemsetAsync(d.fscore.p, 0xFF, sizeof(float) * nf, c->stream)); }
    PCE_HIP(c, hipMemsetAsync(d.score.p, 0xFF, sizeof(float) * n, c->stream));

    for (const Launch &l : launches) {
        const int *lids = d.ids.as<int>() + l.first;
        double cells = 0.0;
        for (size_t x = 0; x < l.count; x++) { const CtcClip &cl = tab[(size_t)ids[l.first + x]]; cells += l.kind == 6 ? (double)cl.T : (double)cl.T * (2.0 * cl.L + 1.0); }
        if (l.kind == 0) {
            KernelTimer t(c, PCE_K_CTC, nullptr, cells);
            hipLaunchKernelGGL(k_ctc<false>, dim3((unsigned)div_up((int64_t)l.count, 4)), dim3(256), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tgt.as<int>(),
                               d.tab.as<CtcClip>(), lids, (int)l.count, d.trace.as<unsigned>(), d.fin.as<float>());
        } else if (l.kind <= 4) {
            KernelTimer t(c, PCE_K_CTC, nullptr, cells);
            hipLaunchKernelGGL(k_ctc<true>, dim3((unsigned)l.count), dim3((unsigned)(WAVE_SIZE << l.kind)), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tgt.as<int>(),
                               d.tab.as<CtcClip>(), lids, (int)l.count, d.trace.as<unsigned>(), d.fin.as<float>());
        } else if (l.kind == 5) {
            KernelTimer t(c, PCE_K_CTC_GENERAL, nullptr, cells);
            hipLaunchKernelGGL(k_ctc_general, dim3((unsigned)l.count), dim3(CTC_GEN_THREADS), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tgt.as<int>(),
                               d.tab.as<CtcClip>(), lids, d.trace.as<unsigned char>(), d.scratch.as<float>(), d.fin.as<float>());
        } else {
            KernelTimer t(c, PCE_K_CTC_TRACE, nullptr, cells);
            hipLaunchKernelGGL(k_ctc_trace, dim3((unsigned)l.count), dim3(WAVE_SIZE), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tgt.as<int>(),
                               d.tab.as<CtcClip>(), lids, d.trace.as<unsigned char>(), d.fin.as<float>(), path ? d.path.as<int>() : nullptr,
                               frame_score ? d.fscore.as<float>() : nullptr, d.first.as<int>(), d.last.as<int>(), d.score.as<float>(), d.status.as<int>());
        }
        PCE_HIP(c, hipGetLastError());
    }
    if (nf && path) PCE_FETCH(c, path, d.path.p, nf);
    if (nf && frame_score) PCE_FETCH(c, frame_score, d.fscore.p, nf);
    if (n_tok) {
        PCE_FETCH(c, tok_first, d.first.p, n_tok);
        PCE_FETCH(c, tok_last, d.last.p, n_tok);
    }
    PCE_FETCH(c, score, d.score.p, n);
    PCE_FETCH(c, status, d.status.p, n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    // a clip without a path: path -1, frame_score NaN, token frames -1; score NaN unless the sweep ran (PCE_CTC_NO_PATH keeps its final value)
    for (size_t q = 0; q < n; q++) {
        if (status[q] == PCE_CTC_OK) continue;
        const CtcClip &cl = tab[q];
        for (int t = 0; t < cl.T; t++) { if (path) path[cl.out0 + t] = -1; if (frame_score) frame_score[cl.out0 + t] = NAN; }
        for (int l = 0; l < cl.L; l++) { tok_first[cl.tgt0 + l] = -1; tok_last[cl.tgt0 + l] = -1; }
        if (status[q] != PCE_CTC_NO_PATH) score[q] = NAN;
    }
    return PCE_OK;
}

} // extern "C"
