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
// k_ctc<false / true>  REGISTER FORM: the register sweep of pce_sweep.h, up to CTC_REG_STATES states.  CTC_RUN is even, so a thread's first state is
//     a blank: it needs alpha[i - 1] only, and the thread's second state takes the same value as its alpha[i - 2]: one value crosses between
//     threads.  The one-frame prefetch is waited for at the end of frame t (in <true>, by sweep_publish's wait in front of the barrier, which
//     also drains the trace store): a frame costs at least max(its arithmetic, one load latency).
// k_ctc_general        GENERAL FORM, any L: one workgroup per clip, the two alpha rows in HBM scratch, threads loop over chunks of states.  Slow, correct.
// k_ctc_trace          one wave per clip, lane 0 walks the back-pointers from the final state to t = 0 and writes path, frame_score, tok_first,
//     tok_last, score and status.
//
// Trace: 2 bits per state, the CTC_RUN states of a thread in one byte, four frames of a thread in one 32-bit word: word (t / 4) * NT + thread
// (NT = threads that sweep the clip), so a wave stores 256 contiguous bytes every fourth frame.  The general form writes the same layout by bytes.
// Clips run in groups whose traces fit PCE_CTC_TRACE_MB MiB (read at pce_create); a clip's outputs depend on its own emissions and targets only.
#include "pce_internal.h"
#include "pce_sweep.h"
#include <cmath>

namespace {

constexpr int CTC_RUN = SWEEP_RUN;                          // states per thread (one trace byte)
static_assert(CTC_RUN % 2 == 0 && CTC_RUN >= 2, "a thread's first state must be a blank: only then does one value cross between threads");
constexpr int CTC_REG_STATES = PCE_CTC_REG_STATES;          // the register form's limit
static_assert(CTC_REG_STATES == CTC_RUN * SWEEP_MAX_THREADS, "include/pce.h states the register form's limit");
constexpr int CTC_GEN_THREADS = 256;
// SweepClip here: n = L targets; stride = NT, the threads (register form) or groups of CTC_RUN states (general form) per frame of trace

__device__ __forceinline__ void ctc_choose(float x0, float x1, float x2, float &chosen, unsigned &bp)
{
    if (x2 > x1 && x2 > x0) { chosen = x2; bp = 2u; }
    else if (x1 > x0 && x1 > x2) { chosen = x1; bp = 1u; }
    else { chosen = x0; bp = 0u; }
}

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? SWEEP_MAX_THREADS : 256) PCE_NO_PK_F32 void k_ctc(const float *__restrict__ lp, int V, int blank, const int *__restrict__ targets,
                                                                                       const SweepClip *__restrict__ clips, const int *__restrict__ ids, int n_ids,
                                                                                       unsigned *__restrict__ trace, float *__restrict__ fin)
{
    __shared__ SweepXch xch;
    const SweepWho who = sweep_who<MULTI>();
    const int lane = who.lane, wave = who.wave, tid = who.tid;
    if (who.slot >= n_ids) return;                           // (<false> only: a whole wave leaves, and that form has no barrier)
    const int c = ids[who.slot];
    const SweepClip cl = clips[c];
    const int S = 2 * cl.n + 1, T = cl.T, NT = cl.stride;
    const int *tg = targets + cl.seq0;
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
    sweep_publish<MULTI>(a[CTC_RUN - 1], xch, 0, lane, wave);
    unsigned word = 0u;
    for (int t = 1; t < T; t++) {
        row += V;
        if (t + 1 < T) {                                     // frame t + 1's emissions: in flight while frame t is computed
#pragma unroll
            for (int k = 0; k < CTC_RUN; k++) en[k] = row[lab[k]];
        }
        const float p1 = sweep_left<MULTI>(a[CTC_RUN - 1], xch, (t - 1) & 1, lane, wave);       // alpha[i0 - 1]: the last state of the thread before
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
        sweep_publish<MULTI>(a[CTC_RUN - 1], xch, t & 1, lane, wave);
        word |= byte << (8 * (t & 3));
        if ((t & 3) == 3 || t == T - 1) {
            if (tid < NT) trace[cl.st0 + (long long)(t >> 2) * NT + tid] = word;
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
                                                                               const SweepClip *__restrict__ clips, const int *__restrict__ ids,
                                                                               unsigned char *__restrict__ trace, float *__restrict__ scratch, float *__restrict__ fin)
{
    const int c = ids[blockIdx.x];
    const SweepClip cl = clips[c];
    const int S = 2 * cl.n + 1, T = cl.T, NT = cl.stride;
    const int *tg = targets + cl.seq0;
    const float NINF = -INFINITY;
    float *A = scratch + cl.scr0, *B = A + S;
    const float *row = lp + cl.row0 * (long long)V;
    for (int i = threadIdx.x; i < S; i += CTC_GEN_THREADS) A[i] = i < 2 ? row[(i & 1) ? tg[0] : blank] : NINF;
    sweep_barrier();
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
            trace[(cl.st0 + (long long)(t >> 2) * NT + g) * 4 + (t & 3)] = (unsigned char)byte;
        }
        sweep_barrier();                                     // (workgroup-scope release / acquire of the row just written)
        float *x = A; A = B; B = x;
    }
    if (threadIdx.x == 0) { fin[2 * c + 1] = A[S - 1]; fin[2 * c] = A[S - 2]; }
}

__global__ __launch_bounds__(WAVE_SIZE) void k_ctc_trace(const float *__restrict__ lp, int V, int blank, const int *__restrict__ targets,
                                                         const SweepClip *__restrict__ clips, const int *__restrict__ ids, const unsigned char *__restrict__ trace,
                                                         const float *__restrict__ fin, int *__restrict__ path, float *__restrict__ frame_score,
                                                         int *__restrict__ tok_first, int *__restrict__ tok_last, float *__restrict__ score, int *__restrict__ status)
{
    if (threadIdx.x != 0) return;
    const int c = ids[blockIdx.x];
    const SweepClip cl = clips[c];
    const int T = cl.T, NT = cl.stride;
    const int *tg = targets + cl.seq0;
    const float f0 = fin[2 * c], f1 = fin[2 * c + 1];
    int i = f1 > f0 ? 2 * cl.n : 2 * cl.n - 1;
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
            const unsigned byte = trace[(cl.st0 + (long long)(t >> 2) * NT + (i >> 2)) * 4 + (t & 3)];
            before = i - (int)((byte >> (2 * (i & 3))) & 3u);       // (state 0 only ever stays, state 1 never takes alpha[i - 2]: before >= 0)
        }
        if (i & 1) {
            if (i != later) tok_last[cl.seq0 + (i >> 1)] = t;
            if (t == 0 || before != i) tok_first[cl.seq0 + (i >> 1)] = t;
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
    const char *fn = "pce_ctc_align";
    PCE_TRY(pce_sweep_check(c, fn, row_start, n_frames, target_off, p, score, status, n_clips, n_vocab, p ? p->blank : 0));
    if (p->form < 0 || p->form > 2) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: form %d (0 auto, 1 register, 2 general)", p->form);
    const size_t n = (size_t)n_clips;
    SweepScan scan;
    std::vector<SweepClip> tab(n);
    std::vector<int> kind(n, -1);                            // -1: not run; 0 .. 4: sweep_kind of the register form; 5: general form
    std::vector<int64_t> words(n, -1);                       // trace words of a clip that runs
    int64_t scratch_floats = 0;
    for (size_t q = 0; q < n; q++) {
        SweepClip &cl = tab[q];
        PCE_TRY(pce_sweep_scan_clip(c, fn, "target", q, row_start, n_frames, target_off, scan, cl));
        const int64_t L = target_off[q + 1] - target_off[q], T = cl.T;
        if (L > 0x3fffffff) return pce_fail(c, PCE_E_LIMIT, "pce_ctc_align: clip %zu has more than 2^30 targets", q);
        if (L && !targets) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: targets is NULL");
        int64_t R = 0;
        for (int64_t l = 0; l < L; l++) {
            const int32_t id = targets[target_off[q] + l];
            if (id < 0 || id >= n_vocab || id == p->blank)
                return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: target %lld of clip %zu is %d (vocabulary %d, blank %d)", (long long)l, q, id, n_vocab, p->blank);
            if (l && id == targets[target_off[q] + l - 1]) R++;
        }
        status[q] = (L == 0 || T == 0) ? PCE_CTC_EMPTY : (T < L + R ? PCE_CTC_TOO_SHORT : PCE_CTC_OK);
        if (status[q] != PCE_CTC_OK) continue;
        const int64_t S = 2 * L + 1, threads = div_up(S, CTC_RUN);
        if (p->form == 1 && S > CTC_REG_STATES)
            return pce_fail(c, PCE_E_LIMIT, "pce_ctc_align: clip %zu has %lld states, the register form holds %d", q, (long long)S, CTC_REG_STATES);
        if (p->form == 2 || S > CTC_REG_STATES) { kind[q] = 5; cl.stride = (int)threads; cl.scr0 = scratch_floats; scratch_floats += 2 * S; }
        else { kind[q] = sweep_kind(threads); cl.stride = WAVE_SIZE << kind[q]; }
        words[q] = div_up(T, 4) * (int64_t)cl.stride;
    }
    if ((scan.total_frames && !emissions) || (target_off[n] && (!tok_first || !tok_last))) return pce_fail(c, PCE_E_INVALID, "pce_ctc_align: NULL emissions or token outputs");
    const SweepGroups groups = sweep_groups(words, (int64_t)(c->sw.ctc_trace_budget / 4));       // consecutive clips whose traces fit the budget
    if (const size_t q = (size_t)groups.too_large; groups.too_large >= 0)
        return pce_fail(c, PCE_E_LIMIT, "pce_ctc_align: clip %zu (%d frames, %d targets) needs %.1f MiB of trace, the budget is %.1f MiB (PCE_CTC_TRACE_MB)", q, tab[q].T,
                        tab[q].n, words[q] * 4.0 / 1048576.0, c->sw.ctc_trace_budget / 1048576.0);
    for (size_t q = 0; q < n; q++) tab[q].st0 = groups.offset[q];

    PCE_HIP(c, hipSetDevice(c->device));
    auto &d = c->ctc;
    const size_t n_tok = (size_t)target_off[n], nf = (size_t)scan.total_frames;
    const float *d_lp;
    PCE_TRY(pce_sweep_stage_emissions(c, d.lp, emissions, emissions_on_device, n_vocab, scan, tab, &d_lp));
    std::vector<int> ids; ids.reserve(n);
    const std::vector<SweepLaunch> launches = sweep_launches(kind, groups.group_end, 6, 6, ids);      // kind 6: the trace walk of a group
    PCE_HIP(c, d.fin.reserve(sizeof(float) * 2 * n));
    PCE_HIP(c, d.trace.reserve(sizeof(unsigned) * (size_t)(groups.largest + 1))); PCE_HIP(c, d.scratch.reserve(sizeof(float) * (size_t)(scratch_floats + 1)));
    PCE_HIP(c, d.path.reserve(sizeof(int) * (nf + 1))); PCE_HIP(c, d.fscore.reserve(sizeof(float) * (nf + 1)));
    PCE_HIP(c, d.first.reserve(sizeof(int) * (n_tok + 1))); PCE_HIP(c, d.last.reserve(sizeof(int) * (n_tok + 1)));
    PCE_HIP(c, d.score.reserve(sizeof(float) * n));
    PCE_UPLOAD(c, d.tab, tab); PCE_UPLOAD(c, d.ids, ids, 1); PCE_UPLOAD(c, d.tgt, targets, n_tok, 1); PCE_UPLOAD(c, d.status, status, (size_t)n);
    if (n_tok) { PCE_HIP(c, hipMemsetAsync(d.first.p, 0xFF, sizeof(int) * n_tok, c->stream)); PCE_HIP(c, hipMemsetAsync(d.last.p, 0xFF, sizeof(int) * n_tok, c->stream)); }
    if (nf) { PCE_HIP(c, hipMemsetAsync(d.path.p, 0xFF, sizeof(int) * nf, c->stream)); PCE_HIP(c, hipMemsetAsync(d.fscore.p, 0xFF, sizeof(float) * nf, c->stream)); }
    PCE_HIP(c, hipMemsetAsync(d.score.p, 0xFF, sizeof(float) * n, c->stream));

    for (const SweepLaunch &l : launches) {
        const int *lids = d.ids.as<int>() + l.first;
        double cells = 0.0;
        for (size_t x = 0; x < l.count; x++) { const SweepClip &cl = tab[(size_t)ids[l.first + x]]; cells += l.kind == 6 ? (double)cl.T : (double)cl.T * (2.0 * cl.n + 1.0); }
        if (l.kind == 0) {
            KernelTimer t(c, PCE_K_CTC, nullptr, cells);
            hipLaunchKernelGGL(k_ctc<false>, dim3((unsigned)div_up((int64_t)l.count, 4)), dim3(256), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tgt.as<int>(),
                               d.tab.as<SweepClip>(), lids, (int)l.count, d.trace.as<unsigned>(), d.fin.as<float>());
        } else if (l.kind <= 4) {
            KernelTimer t(c, PCE_K_CTC, nullptr, cells);
            hipLaunchKernelGGL(k_ctc<true>, dim3((unsigned)l.count), dim3((unsigned)(WAVE_SIZE << l.kind)), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tgt.as<int>(),
                               d.tab.as<SweepClip>(), lids, (int)l.count, d.trace.as<unsigned>(), d.fin.as<float>());
        } else if (l.kind == 5) {
            KernelTimer t(c, PCE_K_CTC_GENERAL, nullptr, cells);
            hipLaunchKernelGGL(k_ctc_general, dim3((unsigned)l.count), dim3(CTC_GEN_THREADS), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tgt.as<int>(),
                               d.tab.as<SweepClip>(), lids, d.trace.as<unsigned char>(), d.scratch.as<float>(), d.fin.as<float>());
        } else {
            KernelTimer t(c, PCE_K_CTC_TRACE, nullptr, cells);
            hipLaunchKernelGGL(k_ctc_trace, dim3((unsigned)l.count), dim3(WAVE_SIZE), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tgt.as<int>(),
                               d.tab.as<SweepClip>(), lids, d.trace.as<unsigned char>(), d.fin.as<float>(), path ? d.path.as<int>() : nullptr,
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
        const SweepClip &cl = tab[q];
        for (int t = 0; t < cl.T; t++) { if (path) path[cl.out0 + t] = -1; if (frame_score) frame_score[cl.out0 + t] = NAN; }
        for (int l = 0; l < cl.n; l++) { tok_first[cl.seq0 + l] = -1; tok_last[cl.seq0 + l] = -1; }
        if (status[q] != PCE_CTC_NO_PATH) score[q] = NAN;
    }
    return PCE_OK;
}

} // extern "C"
