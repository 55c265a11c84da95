// pce_wx.hip -- whisperX's forced alignment of a batch of transcript segments: its own trellis over the J characters of a segment (no interleaved
// blanks), a wildcard emission for characters the model's dictionary lacks, and a beam-search back-track that reads the trellis values.
//
// The numeric core of Code/Aligners/whisperX.py (whisperx.align -> get_trellis / get_wildcard_emission / backtrack_beam).  whisperx is third
// party and absent: restated from the published source of whisperx 3.3.x alignment.py.  The trellis lines are pinned, bit for bit, to the
// installed torch's CPU operators (tests/test_wx_host.py); the back-track's parity with the package is unpinned.  The specification is the
// comment above pce_wx_align in include/pce.h; in short, per clip with e[T][V], tok[J] (-1 = wildcard), blank, beam width W:
//     wild(t, k) = e[t][k] for k >= 0;  max over v != blank of e[t][v] for k = -1
//     tr[0][0] = 0;  tr[t][0] = fp32(sum_{u = 1..t} (double) e[u][blank]) (fp64 accumulator, frame order: torch.cumsum on float32);
//     tr[0][j] = -inf (j >= 1);  tr[t][0] = +inf for t >= max(0, T - J + 1) when J >= 2, and for every t when J = 1
//     tr[t + 1][j] = max(fp32(tr[t][j] + e[t][blank]), fp32(tr[t][j - 1] + wild(t, tok[j])))      j >= 1, t = 0 .. T - 2
// fp32 adds and a max only (no multiply: no FMA can form).  The back-track moves up to W beams from (J - 1, T - 1) one frame down per step;
// a beam at (j, t) offers stay = (j, t - 1) and change = (j - 1, t - 1) where those trellis cells are not +-inf; the candidates are ordered
// by trellis value, descending and STABLE (emission order breaks ties: stay of (t, j) and change of (t, j + 1) land on one cell, so ties are
// structural), the first W survive; it ends when the first beam reaches token 0 (frames below keep token 0) or when no beam is left (NO_PATH).
//
// k_wx_rowmax          wmax[frame] = max over v != blank of e[frame][v], for the frames of the clips that hold a wildcard.  16 lanes per frame,
//     one DPP row tree; a max is order-free, so the value is exact.  It keeps the V-wide reduction off the serial chain of the sweep.
// k_wx_trellis<false / true>   the register sweep of pce_sweep.h over tokens; a frame's emissions are the tok gather, e[t + 1][blank] and
//     wmax[t + 1].  Column 0 (the fp64 prefix of the blank column and the wedge) is produced by the thread that owns token 0, from the same
//     prefetched e[t + 1][blank].  Each frame's row leaves as one 16-byte store per thread: the device table has rows of JP = J rounded up
//     to 4 floats.  Up to PCE_WX_MAX_TOKENS tokens; there is no general form (whisperX aligns segments of at most 30 s: J <= T <= 1 500).
// k_wx_backtrack       one wave per clip.  A beam is its token index (its score is the trellis cell it stands on, all beams share t); beam slot
//     s lives in lane s, candidate i = 2 * slot + (0 stay | 1 change) in lane i < 16.  Every candidate counts the candidates that precede it in
//     the stable descending order (16 lane reads): that count is its place, and it sends its state to the lane of its place (one ds_permute);
//     the first W places are the new beams.  No candidate list is sorted in memory, nothing is indexed dynamically.  This departs from a
//     lane-0 insertion sort: the candidates are independent until they are ranked, so sixteen lanes do in one round what one lane would do in
//     sixteen dependent ones.  The trellis cells come from a prefetched chunk: a step lowers a token by at most one, so the cells the next 7
//     steps can ask for are the offsets 0 .. 7 below the 8 slots' tokens -- 64 (slot, offset) pairs, one per lane, 7 independent loads per lane
//     in flight together instead of one dependent load per step; a beam carries (origin slot, offset) to name its cell.  Measured
//     (profiles/r20/wx_rate.txt): 1.02 -> 0.50 ms for 256 clips x 500 frames with the chunk and the walk below.  Per step and slot it records
//     (token, parent slot), 8 words per frame; the walk up from the winner loads 64 frames' records into registers and follows the parent
//     slots by lane reads (no dependent load per frame), then all lanes write path_tok and path_lp (copies of the emission the move consumed:
//     no exp on the device).
//
// k_wx_trellis is marked PCE_NO_PK_F32 as k_ctc is (its adds could pair; pce_sweep.h keeps it free of calls).  The other two hold no fp32 arithmetic
// a packed instruction could form (a max, compares), and the attribute would keep the runtime's helpers (__ballot, make_int4) out of line in them.
//
// Clips run in groups of consecutive clips whose tables fit PCE_CTC_TRACE_MB MiB together (read at pce_create); a clip's outputs depend on
// its own emissions and tokens only.
#include "pce_internal.h"
#include "pce_sweep.h"
#include <cmath>

namespace {

constexpr int WX_RUN = SWEEP_RUN;                           // tokens per thread: one 16-byte store per frame
static_assert(PCE_WX_MAX_TOKENS == WX_RUN * SWEEP_MAX_THREADS, "include/pce.h states the sweep's limit");
constexpr int WX_SLOTS = PCE_WX_MAX_BEAM;                   // beam slots, and words of back-track record per frame
static_assert(WX_SLOTS == 8, "a record packs the parent slot in 3 bits; 2 * WX_SLOTS candidates fit one DPP row");
constexpr int WX_CHUNK = 7;                                 // back-track steps per prefetched chunk: offsets 0 .. WX_CHUNK x WX_SLOTS origins = one wave

// SweepClip here: n = J tokens; stride = JP, the floats per table row (J rounded up to WX_RUN: st0 is a multiple of 4); out0 also counts wmax

// torch.maximum on the CPU: NaN if either is NaN, else std::max(a, b)
__device__ __forceinline__ float wx_max(float a, float b) { return (a < b || b != b) ? b : a; }

__global__ __launch_bounds__(256) void k_wx_rowmax(const float *__restrict__ lp, int V, int blank, const SweepClip *__restrict__ clips, const int *__restrict__ ids,
                                                   float *__restrict__ wmax)
{
    const SweepClip cl = clips[ids[blockIdx.y]];
    const int f = (int)blockIdx.x * 16 + (int)(threadIdx.x >> 4), l = threadIdx.x & 15;
    if (f >= cl.T) return;                                   // (a whole DPP row leaves: f is one value per 16 lanes)
    const float *row = lp + (cl.row0 + f) * (long long)V;
    float m = -INFINITY;
    for (int v = l; v < V; v += 16) if (v != blank) m = fmaxf(m, row[v]);
    m = dpp_row_max<16>(m);
    if (l == 0) wmax[cl.out0 + f] = m;
}

template <bool MULTI>
__global__ __launch_bounds__(MULTI ? SWEEP_MAX_THREADS : 256) PCE_NO_PK_F32 void k_wx_trellis(const float *__restrict__ lp, int V, int blank, const int *__restrict__ tokens,
                                                                                           const float *__restrict__ wmax, const SweepClip *__restrict__ clips,
                                                                                           const int *__restrict__ ids, int n_ids, float *__restrict__ table)
{
    __shared__ SweepXch xch;
    const SweepWho who = sweep_who<MULTI>();
    const int lane = who.lane, wave = who.wave, tid = who.tid;
    if (who.slot >= n_ids) return;                           // (<false> only: a whole wave leaves, and that form has no barrier)
    const SweepClip cl = clips[ids[who.slot]];
    const int T = cl.T, J = cl.n, JP = cl.stride;
    const int *tk = tokens + cl.seq0;
    const float NINF = -INFINITY, PINF = INFINITY;
    const int wedge = J >= 2 ? max(0, T - J + 1) : 0;        // column 0 is +inf from this frame on
    const bool stores = tid * WX_RUN < JP, col0 = tid == 0;

    int lab[WX_RUN];
    bool live[WX_RUN], star[WX_RUN];
#pragma unroll
    for (int k = 0; k < WX_RUN; k++) {
        const int j = tid * WX_RUN + k;
        live[k] = j < J;
        const int own = live[k] ? tk[j] : blank;
        star[k] = own < 0;
        lab[k] = star[k] ? blank : own;                      // (a wildcard's gather reads a valid column and is replaced by wmax)
    }
    const float *row = lp + cl.row0 * (long long)V;
    const float *wm = wmax + cl.out0;
    float *out = table + cl.st0 + (long long)tid * WX_RUN;
    float a[WX_RUN], w[WX_RUN], wn[WX_RUN];
#pragma unroll
    for (int k = 0; k < WX_RUN; k++) a[k] = NINF;
    if (col0) a[0] = wedge <= 0 ? PINF : 0.0f;
    float eb = row[blank], ebn = 0.0f;
    {
        const float m = cl.wild ? wm[0] : 0.0f;
#pragma unroll
        for (int k = 0; k < WX_RUN; k++) { const float g = row[lab[k]]; w[k] = star[k] ? m : g; wn[k] = 0.0f; }
    }
    if (stores) sweep_store4(out, a);
    sweep_publish<MULTI>(a[WX_RUN - 1], xch, 0, lane, wave);
    double c = 0.0;                                          // the blank column's prefix, frames 1 .. t
    for (int t = 0; t + 1 < T; t++) {
        row += V;
        {                                                    // frame t + 1's emissions: in flight while frame t is computed
            ebn = row[blank];
            const float m = cl.wild ? wm[t + 1] : 0.0f;
#pragma unroll
            for (int k = 0; k < WX_RUN; k++) { const float g = row[lab[k]]; wn[k] = star[k] ? m : g; }
        }
        const float p1 = sweep_left<MULTI>(a[WX_RUN - 1], xch, t & 1, lane, wave);             // tr[t][j0 - 1]: the last token of the thread before
        float na[WX_RUN];
#pragma unroll
        for (int k = 0; k < WX_RUN; k++) {
            const float left = k >= 1 ? a[k - 1] : p1;
            na[k] = live[k] ? wx_max(a[k] + eb, left + w[k]) : NINF;
        }
        c += (double)ebn;
        if (col0) na[0] = (t + 1 >= wedge) ? PINF : (float)c;
#pragma unroll
        for (int k = 0; k < WX_RUN; k++) { a[k] = na[k]; w[k] = wn[k]; }
        eb = ebn;
        sweep_publish<MULTI>(a[WX_RUN - 1], xch, (t + 1) & 1, lane, wave);
        if (stores) sweep_store4(out + (long long)(t + 1) * JP, a);
    }
}

// the place of a trellis value in the descending order: an unsigned key that grows with the value (-0 counts as +0, as a float compare has it)
__device__ __forceinline__ unsigned wx_key(float v)
{
    unsigned b = __builtin_bit_cast(unsigned, v);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(WAVE_SIZE) void k_wx_backtrack(const float *__restrict__ lp, int V, int blank, int W, const int *__restrict__ tokens,
                                                            const float *__restrict__ wmax, const SweepClip *__restrict__ clips, const int *__restrict__ ids,
                                                            const float *__restrict__ table, int *__restrict__ rec, int *__restrict__ path_tok,
                                                            float *__restrict__ path_lp, float *__restrict__ score, int *__restrict__ status)
{
    const int q = ids[blockIdx.x];
    const SweepClip cl = clips[q];
    const int T = cl.T, J = cl.n, JP = cl.stride, lane = threadIdx.x;
    const float *tr = table + cl.st0;
    const float *e = lp + cl.row0 * (long long)V;
    const int *tk = tokens + cl.seq0;
    int *rc = rec + cl.out0 * WX_SLOTS;
    if (lane == 0) score[q] = tr[(long long)(T - 1) * JP + (J - 1)];

    // Beam slot s lives in lane s < WX_SLOTS, packed: token << 9 | parent slot << 6 | origin slot << 3 | offset; -1: no beam.  Origin and offset
    // name the beam's cell inside the chunk's cache: the beam descends from slot `origin` of the chunk's first frame and stands `offset` tokens
    // below that slot's token (a step lowers a token by at most one).
    int st = lane == 0 ? (J - 1) << 9 : -1;
    int t = T - 1, j0 = J - 1;
    bool any = true;
    while (any && j0 > 0 && t > 0) {
        // a chunk of WX_CHUNK steps: lane (o, d) = (lane >> 3, lane & 7) loads, for each of the next rows, the cell d tokens below slot o's token --
        // every cell the chunk can ask for, WX_CHUNK independent loads per lane in flight together instead of one dependent load per step
        st = st < 0 ? -1 : (((st >> 9) << 9) | (lane << 3));
        const int oj = __shfl(st, lane >> 3, WAVE_SIZE) >> 9, d = lane & 7;
        float cache[WX_CHUNK];
#pragma unroll
        for (int r = 0; r < WX_CHUNK; r++) {
            const int row = t - 1 - r, col = oj - d;
            cache[r] = (oj >= 0 && row >= 0 && col >= 0 && d <= r + 1) ? tr[(long long)row * JP + col] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < WX_CHUNK; r++) {
            if (any && j0 > 0 && t > 0) {                    // (wave-uniform)
                // candidate i = 2 * slot + (0 stay | 1 change) in lane i < 2 * WX_SLOTS: the order the source emits them in
                const int parent = (lane >> 1) & (WX_SLOTS - 1), chg = lane & 1;
                const int ps = __shfl(st, parent, WAVE_SIZE);
                const int cj = (ps >> 9) - chg, org = (ps >> 3) & 7, off = ((ps & 7) + chg) & 7;
                const float val = __shfl(cache[r], org * 8 + off, WAVE_SIZE);       // tr[t - 1][cj]
                const bool ok = lane < 2 * WX_SLOTS && ps >= 0 && cj >= 0 && fabsf(val) != INFINITY;
                const unsigned key = ok ? max(wx_key(val), 1u) : 0u;                 // 0: no candidate
                int place = 0;                               // candidates before this one: a greater value, or an equal one emitted earlier
#pragma unroll
                for (int k = 0; k < 2 * WX_SLOTS; k++) {
                    const unsigned kk = (unsigned)__builtin_amdgcn_readlane((int)key, k);
                    place += (kk != 0u && (kk > key || (kk == key && k < lane))) ? 1 : 0;
                }
                const int n = __popcll(__ballot(ok));
                // the places of the candidates are a permutation of 0 .. n - 1: each sends its state to the lane of its place (the others to lanes nobody reads)
                const int mine = (cj << 9) | (parent << 6) | (org << 3) | off;
                const int got = __builtin_amdgcn_ds_permute((ok ? place : 48 + (lane & 15)) << 2, mine);
                st = lane < min(n, W) ? got : -1;
                if (lane < WX_SLOTS) rc[(long long)(t - 1) * WX_SLOTS + lane] = st < 0 ? -1 : (((st >> 9) << 3) | ((st >> 6) & 7));
                t--;
                any = n > 0;
                j0 = __builtin_amdgcn_readfirstlane(st) >> 9;
            }
        }
    }
    if (j0 > 0) any = false;                                 // frame 0 above token 0: every beam is dropped
    if (!any) { if (lane == 0) status[q] = PCE_WX_NO_PATH; return; }
    if (lane == 0) status[q] = PCE_WX_OK;
    if (!path_tok && !path_lp) return;
    // the first beam stands on (j0, t): the frames below keep its token, on the blank's emission
    for (int f = lane; f < t; f += WAVE_SIZE) {
        if (path_tok) path_tok[cl.out0 + f] = j0;
        if (path_lp) path_lp[cl.out0 + f] = e[(long long)f * V + blank];
    }
    __threadfence();                                         // (the record was written by other lanes of this wave)
    // The walk up from slot 0 of frame t: lane l holds the eight records of frame f0 + l, the chain of parent slots runs over lane reads (no
    // dependent load per frame); the winner's token of frame f replaces word 0 of that frame's record.
    int cur = 0;
    for (int f0 = t; f0 < T - 1; f0 += WAVE_SIZE) {
        const int f = f0 + lane;
        int4 lo = make_int4(-1, -1, -1, -1), hi = lo;
        if (f < T - 1) {
            const int4 *p = reinterpret_cast<const int4 *>(rc + (long long)f * WX_SLOTS);
            lo = p[0]; hi = p[1];
        }
        const int frames = min(WAVE_SIZE, T - 1 - f0);
        int mine = 0;
        for (int l = 0; l < frames; l++) {
            const int sel = cur == 0 ? lo.x : cur == 1 ? lo.y : cur == 2 ? lo.z : cur == 3 ? lo.w : cur == 4 ? hi.x : cur == 5 ? hi.y : cur == 6 ? hi.z : hi.w;
            const int r = __builtin_amdgcn_readlane(sel, l);
            if (lane == l) mine = r >> 3;
            cur = r & 7;
        }
        if (f < T - 1) rc[(long long)f * WX_SLOTS] = mine;
    }
    __threadfence();
    for (int f = t + lane; f < T; f += WAVE_SIZE) {
        // frame T - 1 is the start: token J - 1 on the blank's emission; a frame whose successor stands one token higher consumed the emission of
        // the token being left
        const int j = f < T - 1 ? rc[(long long)f * WX_SLOTS] : J - 1;
        const int jn = f + 1 < T - 1 ? rc[(long long)(f + 1) * WX_SLOTS] : J - 1;
        if (path_tok) path_tok[cl.out0 + f] = j;
        if (path_lp) {
            float v;
            if (f == T - 1 || jn == j) v = e[(long long)f * V + blank];
            else { const int left = tk[min(max(jn, 0), J - 1)]; v = left < 0 ? wmax[cl.out0 + f] : e[(long long)f * V + left]; }
            path_lp[cl.out0 + f] = v;
        }
    }
}

} // namespace

extern "C" {

int pce_wx_align(pce_ctx *c, const float *emissions, int32_t emissions_on_device, const int64_t *row_start, const int32_t *n_frames, int32_t n_vocab,
                 const int32_t *tokens, const int64_t *token_off, int32_t n_clips, const pce_wx_params *p, int32_t *path_tok, float *path_lp, float *trellis,
                 float *score, int32_t *status)
{
    if (!c) return PCE_E_INVALID;
    const char *fn = "pce_wx_align";
    PCE_TRY(pce_sweep_check(c, fn, row_start, n_frames, token_off, p, score, status, n_clips, n_vocab, p ? p->blank : 0));
    if (p->beam_width < 1 || p->beam_width > PCE_WX_MAX_BEAM)
        return pce_fail(c, PCE_E_INVALID, "pce_wx_align: beam width %d outside 1 .. %d", p->beam_width, PCE_WX_MAX_BEAM);
    const size_t n = (size_t)n_clips;
    SweepScan scan;
    std::vector<SweepClip> tab(n);
    std::vector<int> kind(n, -1);                            // -1: not run; 0 .. 4: sweep_kind
    std::vector<int64_t> floats(n, -1);                      // table floats of a clip that runs
    std::vector<int64_t> cells_off(n + 1, 0);                // floats of the caller's trellis before clip q
    for (size_t q = 0; q < n; q++) {
        SweepClip &cl = tab[q];
        PCE_TRY(pce_sweep_scan_clip(c, fn, "token", q, row_start, n_frames, token_off, scan, cl));
        const int64_t J = token_off[q + 1] - token_off[q], T = cl.T;
        if (J > PCE_WX_MAX_TOKENS) return pce_fail(c, PCE_E_LIMIT, "pce_wx_align: clip %zu has %lld tokens, the sweep holds %d", q, (long long)J, PCE_WX_MAX_TOKENS);
        if (J && !tokens) return pce_fail(c, PCE_E_INVALID, "pce_wx_align: tokens is NULL");
        for (int64_t l = 0; l < J; l++) {
            const int32_t id = tokens[token_off[q] + l];
            if (id < -1 || id >= n_vocab)
                return pce_fail(c, PCE_E_INVALID, "pce_wx_align: token %lld of clip %zu is %d (vocabulary %d, -1 = wildcard)", (long long)l, q, id, n_vocab);
            if (id < 0) cl.wild = 1;
        }
        cl.stride = (int)(div_up(J, WX_RUN) * WX_RUN);
        cells_off[q + 1] = cells_off[q] + T * J;
        status[q] = (J == 0 || T == 0) ? PCE_WX_EMPTY : PCE_WX_OK;
        if (status[q] != PCE_WX_OK) continue;
        kind[q] = sweep_kind(div_up(J, WX_RUN));
        floats[q] = T * cl.stride;
    }
    if (scan.total_frames && !emissions) return pce_fail(c, PCE_E_INVALID, "pce_wx_align: NULL emissions");
    const SweepGroups groups = sweep_groups(floats, (int64_t)(c->sw.ctc_trace_budget / 4));      // consecutive clips whose tables fit the budget
    if (const size_t q = (size_t)groups.too_large; groups.too_large >= 0)
        return pce_fail(c, PCE_E_LIMIT, "pce_wx_align: clip %zu (%d frames, %d tokens) needs %.1f MiB of trellis, the budget is %.1f MiB (PCE_CTC_TRACE_MB)", q, tab[q].T,
                        tab[q].n, floats[q] * 4.0 / 1048576.0, c->sw.ctc_trace_budget / 1048576.0);
    for (size_t q = 0; q < n; q++) tab[q].st0 = groups.offset[q];

    PCE_HIP(c, hipSetDevice(c->device));
    auto &d = c->wx;
    const size_t n_tok = (size_t)token_off[n], nf = (size_t)scan.total_frames;
    const float *d_lp;
    PCE_TRY(pce_sweep_stage_emissions(c, d.lp, emissions, emissions_on_device, n_vocab, scan, tab, &d_lp));
    // id lists: the clips with a wildcard first, then per group, per kind
    std::vector<int> ids; ids.reserve(2 * n);
    int max_wild_T = 0;
    for (size_t q = 0; q < n; q++) if (kind[q] >= 0 && tab[q].wild) { ids.push_back((int)q); max_wild_T = std::max(max_wild_T, tab[q].T); }
    const size_t n_wild = ids.size();
    const std::vector<SweepLaunch> launches = sweep_launches(kind, groups.group_end, 5, 5, ids);      // kind 5: the back-track of a group
    PCE_HIP(c, d.table.reserve(sizeof(float) * (size_t)(groups.largest + 4)));
    PCE_HIP(c, d.wmax.reserve(sizeof(float) * (nf + 1)));
    PCE_HIP(c, d.rec.reserve(sizeof(int) * (nf + 1) * WX_SLOTS));
    PCE_HIP(c, d.path.reserve(sizeof(int) * (nf + 1))); PCE_HIP(c, d.plp.reserve(sizeof(float) * (nf + 1)));
    PCE_HIP(c, d.score.reserve(sizeof(float) * n));
    PCE_UPLOAD(c, d.tab, tab); PCE_UPLOAD(c, d.ids, ids, 1); PCE_UPLOAD(c, d.tok, tokens, n_tok, 1); PCE_UPLOAD(c, d.status, status, (size_t)n);
    if (nf) { PCE_HIP(c, hipMemsetAsync(d.path.p, 0xFF, sizeof(int) * nf, c->stream)); PCE_HIP(c, hipMemsetAsync(d.plp.p, 0xFF, sizeof(float) * nf, c->stream)); }
    PCE_HIP(c, hipMemsetAsync(d.score.p, 0xFF, sizeof(float) * n, c->stream));

    if (n_wild) {
        double cells = 0.0;
        for (size_t x = 0; x < n_wild; x++) cells += (double)tab[(size_t)ids[x]].T * n_vocab;
        KernelTimer t(c, PCE_K_WX_ROWMAX, nullptr, cells);
        hipLaunchKernelGGL(k_wx_rowmax, dim3((unsigned)div_up(max_wild_T, 16), (unsigned)n_wild), dim3(256), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank,
                           d.tab.as<SweepClip>(), d.ids.as<int>(), d.wmax.as<float>());
        PCE_HIP(c, hipGetLastError());
    }
    for (const SweepLaunch &l : launches) {
        const int *lids = d.ids.as<int>() + l.first;
        double cells = 0.0;
        for (size_t x = 0; x < l.count; x++) { const SweepClip &cl = tab[(size_t)ids[l.first + x]]; cells += l.kind == 5 ? (double)cl.T : (double)cl.T * cl.n; }
        if (l.kind == 0) {
            KernelTimer t(c, PCE_K_WX_TRELLIS, nullptr, cells);
            hipLaunchKernelGGL(k_wx_trellis<false>, dim3((unsigned)div_up((int64_t)l.count, 4)), dim3(256), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, d.tok.as<int>(),
                               d.wmax.as<float>(), d.tab.as<SweepClip>(), lids, (int)l.count, d.table.as<float>());
        } else if (l.kind <= 4) {
            KernelTimer t(c, PCE_K_WX_TRELLIS, nullptr, cells);
            hipLaunchKernelGGL(k_wx_trellis<true>, dim3((unsigned)l.count), dim3((unsigned)(WAVE_SIZE << l.kind)), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank,
                               d.tok.as<int>(), d.wmax.as<float>(), d.tab.as<SweepClip>(), lids, (int)l.count, d.table.as<float>());
        } else {
            {
                KernelTimer t(c, PCE_K_WX_BACKTRACK, nullptr, cells);
                hipLaunchKernelGGL(k_wx_backtrack, dim3((unsigned)l.count), dim3(WAVE_SIZE), 0, c->stream, d_lp, (int)n_vocab, (int)p->blank, (int)p->beam_width,
                                   d.tok.as<int>(), d.wmax.as<float>(), d.tab.as<SweepClip>(), lids, d.table.as<float>(), d.rec.as<int>(),
                                   path_tok ? d.path.as<int>() : nullptr, path_lp ? d.plp.as<float>() : nullptr, d.score.as<float>(), d.status.as<int>());
            }
            PCE_HIP(c, hipGetLastError());
            // the stage hook: the group's tables leave before the next group overwrites them (rows of JP floats on the device, of J for the caller)
            if (trellis) {
                for (size_t q = l.g0; q < l.ge; q++) {
                    if (kind[q] < 0) continue;
                    const SweepClip &cl = tab[q];
                    PCE_HIP(c, hipMemcpy2DAsync(trellis + cells_off[q], sizeof(float) * (size_t)cl.n, d.table.as<float>() + cl.st0, sizeof(float) * (size_t)cl.stride,
                                                sizeof(float) * (size_t)cl.n, (size_t)cl.T, hipMemcpyDeviceToHost, c->stream));
                }
            }
        }
        PCE_HIP(c, hipGetLastError());
    }
    if (nf && path_tok) PCE_FETCH(c, path_tok, d.path.p, nf);
    if (nf && path_lp) PCE_FETCH(c, path_lp, d.plp.p, nf);
    PCE_FETCH(c, score, d.score.p, n);
    PCE_FETCH(c, status, d.status.p, n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    // a clip without a path: path_tok -1, path_lp NaN; score NaN unless the sweep ran (PCE_WX_NO_PATH keeps the final trellis cell)
    for (size_t q = 0; q < n; q++) {
        if (status[q] == PCE_WX_OK) continue;
        const SweepClip &cl = tab[q];
        for (int t = 0; t < cl.T; t++) { if (path_tok) path_tok[cl.out0 + t] = -1; if (path_lp) path_lp[cl.out0 + t] = NAN; }
        if (status[q] != PCE_WX_NO_PATH) score[q] = NAN;
    }
    return PCE_OK;
}

} // extern "C"
