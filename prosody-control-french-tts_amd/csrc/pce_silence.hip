// pce_silence.hip -- pydub's detect_silence over slices of the resident batch, in exact integers.
//
// Reference step replaced: pydub.silence.split_on_silence / detect_nonsilent as Code/Preprocessing/preprocess_audio.py:41-46 and
// Code/audioPipeline.py:720,786-797 call them (pydub 0.25.1 is third party and absent: the range bookkeeping is restated from its
// published source, parity unpinned; the window test is pinned to stdlib audioop.rms, the function pydub calls).  pydub takes a
// min_silence_len slice at every seek_step and calls audioop.rms on each: O(samples x window).  Here (include/pce.h has the rules):
//   k_ms_energy       the one pass over the PCM: sum of squares of every millisecond bin [b(m), b(m + 1)), and -- the owner of a bin being
//                     a thread of the workgroup that owns the chunk of SI_CHUNK bins -- the exclusive prefix sum INSIDE the chunk and the
//                     chunk's total.  HBM-bound: 2 bytes per sample read once, 8 bytes per millisecond written.
//   k_silence_scan    one wavefront per slice: exclusive prefix sum of its chunk totals (tiles of 64 with a carry).
//                     P[i] = in-chunk prefix[i] + chunk offset[i / chunk] is what the readers below add up: no third pass over the bins.
//   k_silence_ranges  three launches under one profile id.  <tiles>: a workgroup takes SI_TILE consecutive window starts, tests every window
//                     (P[s + L] - P[s] < (T + 1)^2 n_s), finds each silent start's previous silent start inside the tile (max-scan) and
//                     counts the range openers that need nothing from outside the tile: every silent start but the tile's first.
//                     <carry>: one wavefront per slice carries the last silent start and the opener count across tiles (tiles of 64).
//                     <tiles, final>: the same pass with the carry: opener r writes range r's start and range r - 1's end.
// Everything is integer (uint64 sums, int32 milliseconds) but the boundary b(m) = (int64)((double)m * (rate / 1000.0)), pydub's own product,
// computed with the same fp64 multiply: results cannot depend on the batch or on scheduling.
#include "pce_internal.h"
#include <cmath>

namespace {

constexpr int SI_THREADS = 256;
constexpr int SI_CHUNK_LOG2_MAX = 8;                    // bins per chunk: one per thread at most
constexpr int SI_ITEMS = 4;                             // window starts per thread
constexpr int SI_TILE = SI_THREADS * SI_ITEMS;
constexpr size_t SI_LDS_MAX = 48 << 10;

struct SiSlice {
    int64_t g_base;             // index of the slice's sample 0 in the batch (clip offset + begin: before the clip where begin < 0)
    int64_t jv0, jv1;           // the slice's samples [jv0, jv1) exist in its clip; the others are zeros
    int64_t p_off;              // this slice's first entry in the prefix array (len_ms + 1 entries where it has windows)
    int64_t chunk_off, tile_off, range_off;   // chunks / tiles / output capacity before this slice (entry n_slices: the totals)
    int32_t len_ms, n_starts, n_regular, last, cap, pad;
    unsigned long long thr2;    // (T + 1)^2
};
struct SiTile { int first, last, openers, pad; };       // silent starts of a tile (-1: none), its openers other than `first`
struct SiCarry { int prev, rbase; };                    // last silent start before the tile (-1: none), ranges opened before it

template <class Key> __device__ __forceinline__ int si_find(const SiSlice *sl, int n, int64_t idx, Key key)
{
    int lo = 0, hi = n;                                 // the last slice whose offset is <= idx (slices without work share their successor's offset)
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (key(sl[mid]) <= idx) lo = mid; else hi = mid; }
    return lo;
}

__device__ __forceinline__ unsigned long long si_wave_incl_u64(unsigned long long v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) { const unsigned long long o = __shfl_up(v, off, 64); if (lane >= off) v += o; }
    return v;
}
__device__ __forceinline__ int si_wave_incl_sum(int v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(v, off, 64); if (lane >= off) v += o; }
    return v;
}
__device__ __forceinline__ int si_wave_incl_max(int v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(v, off, 64); if (lane >= off) v = max(v, o); }
    return v;
}

template <bool NT>
__global__ __launch_bounds__(SI_THREADS) void k_ms_energy(const int16_t *__restrict__ pcm, const SiSlice *__restrict__ sl, int n_slices, double rk, int ch,
                                                         int cb_log2, int lds_words, unsigned long long *__restrict__ pl, unsigned long long *__restrict__ csum)
{
    typedef int i4 __attribute__((ext_vector_type(4)));
    typedef short s2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) int si_lds[];          // [0, 16): hand-off words of the scan; then the chunk's samples
    unsigned long long *l_wave = reinterpret_cast<unsigned long long *>(si_lds);
    int *l_pcm = si_lds + 16;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t chunk = blockIdx.x;
    const SiSlice S = sl[si_find(sl, n_slices, chunk, [](const SiSlice &s) { return s.chunk_off; })];
    const int cb = 1 << cb_log2;
    const int64_t m0 = (chunk - S.chunk_off) << cb_log2;
    const int64_t m1 = m0 + cb < S.len_ms ? m0 + cb : S.len_ms;           // bins [m0, m1); entry len_ms of the prefix array follows the last bin
    auto bnd = [&](int64_t m) -> int64_t { return (int64_t)((double)m * rk) * ch; };
    const int64_t b0 = bnd(m0), b1 = bnd(m1);
    const int64_t ja = b0 > S.jv0 ? b0 : S.jv0, jb = b1 < S.jv1 ? b1 : S.jv1;
    const int64_t ga = (S.g_base + ja) & ~(int64_t)7;                     // 16-byte group of the first sample (>= the clip's first: inside the batch)
    int nvec = jb > ja ? (int)((S.g_base + jb - ga + 7) >> 3) : 0;
    if (nvec * 4 > lds_words) nvec = 0;                                   // (the host sized the region for the widest chunk: never taken)
#pragma unroll 4
    for (int v = tid; v < nvec; v += SI_THREADS) {
        const i4 *p = reinterpret_cast<const i4 *>(pcm + ga + (int64_t)v * 8);
        *reinterpret_cast<i4 *>(l_pcm + v * 4) = NT ? __builtin_nontemporal_load(p) : *p;
    }
    __syncthreads();
    const int64_t m = m0 + tid;
    unsigned long long e = 0;
    if (tid < cb && m < m1 && nvec > 0) {
        const int64_t t0 = bnd(m), t1 = bnd(m + 1);
        const int64_t j0 = t0 > ja ? t0 : ja, j1 = t1 < jb ? t1 : jb;
        if (j1 > j0) {
            const int s0 = (int)(S.g_base + j0 - ga), ns = (int)(j1 - j0);          // samples [s0, s0 + ns) of the staged region
            const int w0 = s0 >> 1, nw = ((s0 + ns + 1) >> 1) - w0;
            // integer sums: a lane may take its words in any order.  Starting a few words in, by lane, spreads the lanes of a wave over the
            // LDS banks where the bins are a power of two long (16 kHz: 8 words per bin, every fourth lane on one bank otherwise)
            int r = (lane >> 2) & 7; if (r >= nw) r = 0;
            for (int i = 0; i < nw; i++) {
                const int w = w0 + r;
                r = r + 1 == nw ? 0 : r + 1;
                const int rel = 2 * w - s0;
                const unsigned keep = ((unsigned)rel < (unsigned)ns ? 0x0000FFFFu : 0u) | ((unsigned)(rel + 1) < (unsigned)ns ? 0xFFFF0000u : 0u);
                const s2 xv = __builtin_bit_cast(s2, (int)((unsigned)l_pcm[w] & keep));
                e += (unsigned long long)(unsigned int)__builtin_amdgcn_sdot2(xv, xv, 0, false);     // <= 2^31: exact as unsigned
            }
        }
    }
    const unsigned long long incl = si_wave_incl_u64(e, lane);
    if (lane == 63) l_wave[wv] = incl;
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int q = 0; q < SI_THREADS / 64; q++) { const unsigned long long t = l_wave[q]; if (q < wv) before += t; total += t; }
    if (tid < cb && m <= S.len_ms) pl[S.p_off + m] = before + incl - e;
    if (tid == 0) csum[chunk] = total;
}

__global__ __launch_bounds__(64) void k_silence_scan(const SiSlice *__restrict__ sl, const unsigned long long *__restrict__ csum,
                                                    unsigned long long *__restrict__ coff)
{
    const int lane = threadIdx.x;
    const int64_t c0 = sl[blockIdx.x].chunk_off, nc = sl[blockIdx.x + 1].chunk_off - c0;
    unsigned long long carry = 0;
    for (int64_t base = 0; base < nc; base += 64) {
        const int64_t i = base + lane;
        const unsigned long long v = i < nc ? csum[c0 + i] : 0;
        const unsigned long long incl = si_wave_incl_u64(v, lane);
        if (i < nc) coff[c0 + i] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
}

// SI_TILE consecutive window starts of one slice: start k is k * step for k < n_regular and `last` (= len_ms - L, where step does not divide it) after them.
template <bool FINAL>
__global__ __launch_bounds__(SI_THREADS) void k_silence_ranges(const SiSlice *__restrict__ sl, int n_slices, double rk, int ch, int cb_log2, int L, int step,
                                                              const unsigned long long *__restrict__ pl, const unsigned long long *__restrict__ coff,
                                                              SiTile *__restrict__ tsum, const SiCarry *__restrict__ tin, int *__restrict__ out)
{
    __shared__ int l_wave[2][SI_THREADS / 64];
    __shared__ int l_first, l_last, l_open;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t tile = blockIdx.x;
    const SiSlice S = sl[si_find(sl, n_slices, tile, [](const SiSlice &s) { return s.tile_off; })];
    const int64_t k0 = (tile - S.tile_off) * SI_TILE + (int64_t)tid * SI_ITEMS;
    if (tid == 0) { l_first = 0x7FFFFFFF; l_last = -1; l_open = 0; }
    auto prefix = [&](int64_t i) -> unsigned long long { return pl[S.p_off + i] + coff[S.chunk_off + (i >> cb_log2)]; };
    auto frames = [&](int64_t ms) -> int64_t { return (int64_t)((double)ms * rk); };
    int st[SI_ITEMS], pin[SI_ITEMS];                    // a silent start and its previous silent start inside this thread (-1: none); st = -1: not silent
    int mine = -1;
#pragma unroll
    for (int j = 0; j < SI_ITEMS; j++) {
        const int64_t k = k0 + j;
        st[j] = -1; pin[j] = mine;
        if (k < S.n_starts) {
            const int s = k < S.n_regular ? (int)(k * step) : S.last;
            const unsigned long long n_s = (unsigned long long)((frames((int64_t)s + L) - frames(s)) * ch);
            if (prefix((int64_t)s + L) - prefix(s) < S.thr2 * n_s) { st[j] = s; mine = s; }
        }
    }
    // exclusive max-scan of the threads' last silent starts
    const int incl = si_wave_incl_max(mine, lane);
    if (lane == 63) l_wave[0][wv] = incl;
    __syncthreads();                                    // (also: the three words above are initialised)
    int prev = __shfl_up(incl, 1, 64); if (lane == 0) prev = -1;
    for (int q = 0; q < wv; q++) prev = max(prev, l_wave[0][q]);
    if (FINAL && prev < 0) prev = tin[tile].prev;
    int n_open = 0; bool open[SI_ITEMS]; int before[SI_ITEMS];
#pragma unroll
    for (int j = 0; j < SI_ITEMS; j++) {
        open[j] = false; before[j] = -1;
        if (st[j] < 0) continue;
        const int p = pin[j] >= 0 ? pin[j] : prev;
        before[j] = p;
        // pydub: a silent start opens a range when it neither continues the previous one nor lies within min_silence_len of it.  Without the
        // carry the tile's first silent start (p < 0) is left to k_silence_carry
        open[j] = p < 0 ? FINAL : (st[j] != p + step && (int64_t)st[j] > (int64_t)p + L);
        n_open += open[j];
    }
    if (!FINAL) {
        if (mine >= 0) {
            int f = -1;
#pragma unroll
            for (int j = SI_ITEMS - 1; j >= 0; j--) if (st[j] >= 0) f = st[j];
            atomicMin(&l_first, f); atomicMax(&l_last, mine);
        }
        if (n_open) atomicAdd(&l_open, n_open);
        __syncthreads();
        if (tid == 0) tsum[tile] = SiTile{l_first == 0x7FFFFFFF ? -1 : l_first, l_last, l_open, 0};
        return;
    }
    const int oincl = si_wave_incl_sum(n_open, lane);
    if (lane == 63) l_wave[1][wv] = oincl;
    __syncthreads();
    int r = tin[tile].rbase + oincl - n_open;
    for (int q = 0; q < wv; q++) r += l_wave[1][q];
#pragma unroll
    for (int j = 0; j < SI_ITEMS; j++) {
        if (!open[j]) continue;
        if (r < S.cap) out[2 * (S.range_off + r)] = st[j];
        if (r >= 1 && r - 1 < S.cap) out[2 * (S.range_off + r - 1) + 1] = before[j] + L;     // (an opener after the first has a silent start before it)
        r++;
    }
}

__global__ __launch_bounds__(64) void k_silence_carry(const SiSlice *__restrict__ sl, int L, int step, const SiTile *__restrict__ tsum,
                                                     SiCarry *__restrict__ tin, int *__restrict__ out, int *__restrict__ count)
{
    const int lane = threadIdx.x;
    const SiSlice S = sl[blockIdx.x];
    const int64_t t0 = S.tile_off, nt = sl[blockIdx.x + 1].tile_off - t0;
    int carry_prev = -1, carry_n = 0;
    for (int64_t base = 0; base < nt; base += 64) {
        const int64_t i = base + lane;
        SiTile t = SiTile{-1, -1, 0, 0};
        if (i < nt) t = tsum[t0 + i];
        const int lincl = si_wave_incl_max(t.last, lane);
        int prev = __shfl_up(lincl, 1, 64); if (lane == 0) prev = -1;
        prev = max(prev, carry_prev);
        const bool opens = t.first >= 0 && (prev < 0 || (t.first != prev + step && (int64_t)t.first > (int64_t)prev + L));
        const int n = t.openers + (opens ? 1 : 0);
        const int nincl = si_wave_incl_sum(n, lane);
        if (i < nt) tin[t0 + i] = SiCarry{prev, carry_n + nincl - n};
        carry_prev = max(carry_prev, __shfl(lincl, 63, 64));
        carry_n += __shfl(nincl, 63, 64);
    }
    if (lane == 0) {
        count[blockIdx.x] = carry_n;
        if (carry_n >= 1 && carry_n <= S.cap) out[2 * (S.range_off + carry_n - 1) + 1] = carry_prev + L;   // the last range ends with the last silent window
    }
}

} // namespace

extern "C" {

int pce_silence_run(pce_ctx *c, const pce_silence_params *p, const pce_slice *slices, const int32_t *rms_max, int32_t n)
{
    if (!c || !p || n < 0 || (n > 0 && (!slices || !rms_max))) return PCE_E_INVALID;
    if (!c->d_pcm) return pce_fail(c, PCE_E_STATE, "no batch uploaded");
    if (p->min_silence_len < 1 || p->seek_step < 1 || p->channels < 1)
        return pce_fail(c, PCE_E_INVALID, "silence: need min_silence_len >= 1, seek_step >= 1, channels >= 1");
    c->si_n = -1;
    const int ch = p->channels, L = p->min_silence_len, step = p->seek_step;
    const double rk = c->rate / 1000.0;
    // bins per chunk: the largest power of two (at most one per thread) whose samples fit the staging region
    auto chunk_words = [&](int cb) -> int64_t { return (((int64_t)((double)cb * rk) + 2) * ch + 16 + 7) / 8 * 4; };
    int cb_log2 = SI_CHUNK_LOG2_MAX;
    while (cb_log2 > 0 && (size_t)(chunk_words(1 << cb_log2) + 16) * 4 > SI_LDS_MAX) cb_log2--;
    if ((size_t)(chunk_words(1 << cb_log2) + 16) * 4 > SI_LDS_MAX)
        return pce_fail(c, PCE_E_LIMIT, "silence: one millisecond of %d Hz x %d channels does not fit the staging region", c->rate, ch);
    std::vector<SiSlice> meta((size_t)n + 1);
    c->si_len_ms.assign((size_t)n, 0); c->si_status.assign((size_t)n, PCE_SLICE_OK); c->si_cap_off.assign((size_t)n + 1, 0);
    int64_t p_off = 0, chunk_off = 0, tile_off = 0, range_off = 0;
    for (int32_t i = 0; i < n; i++) {
        const pce_slice &s = slices[i];
        if (s.clip < 0 || s.clip >= c->n_clips) return pce_fail(c, PCE_E_INVALID, "slice %d: clip %d out of range", i, s.clip);
        if (s.end < s.begin) return pce_fail(c, PCE_E_INVALID, "slice %d: end < begin", i);
        if (rms_max[i] < 0) return pce_fail(c, PCE_E_INVALID, "slice %d: rms_max < 0", i);
        if (s.begin % ch != 0 || s.end % ch != 0) return pce_fail(c, PCE_E_INVALID, "slice %d: bounds are not multiples of %d channels", i, ch);
        const int64_t clip_len = c->clip_off[(size_t)s.clip + 1] - c->clip_off[(size_t)s.clip];
        const int64_t n_frames = (s.end - s.begin) / ch;
        const double len_d = std::nearbyint(1000.0 * ((double)n_frames / (double)c->rate));      // Python's round(): half to even
        if (len_d > 2147483647.0) return pce_fail(c, PCE_E_LIMIT, "slice %d: more than 2^31 - 1 milliseconds", i);
        const int32_t len_ms = (int32_t)len_d;
        SiSlice &m = meta[(size_t)i];
        m.g_base = c->clip_off[(size_t)s.clip] + s.begin;
        m.jv0 = s.begin < 0 ? -s.begin : 0;
        m.jv1 = (s.end < clip_len ? s.end : clip_len) - s.begin;
        m.p_off = p_off; m.chunk_off = chunk_off; m.tile_off = tile_off; m.range_off = range_off;
        m.len_ms = len_ms; m.pad = 0;
        const int64_t t = rms_max[i] < 32768 ? rms_max[i] : 32768;                               // (every window is silent from 32768 on)
        m.thr2 = (unsigned long long)((t + 1) * (t + 1));
        if (n_frames == 0) c->si_status[(size_t)i] = PCE_SLICE_EMPTY;
        if (len_ms >= L) {
            m.last = len_ms - L;
            m.n_regular = m.last / step + 1;
            m.n_starts = m.n_regular + (m.last % step != 0 ? 1 : 0);
            m.cap = len_ms / (L + 1) + 1;
            p_off += (int64_t)len_ms + 1;
            chunk_off += ((int64_t)len_ms + 1 + (1 << cb_log2) - 1) >> cb_log2;
            tile_off += div_up(m.n_starts, SI_TILE);
        } else {
            m.last = 0; m.n_regular = 0; m.n_starts = 0; m.cap = 0;
        }
        range_off += m.cap;
        c->si_len_ms[(size_t)i] = len_ms; c->si_cap_off[(size_t)i + 1] = range_off;
    }
    SiSlice &end = meta[(size_t)n];
    memset(&end, 0, sizeof(end));
    end.p_off = p_off; end.chunk_off = chunk_off; end.tile_off = tile_off; end.range_off = range_off;
    if (chunk_off > 0x7FFFFFFF || tile_off > 0x7FFFFFFF) return pce_fail(c, PCE_E_LIMIT, "silence: more chunks than one launch holds");
    PCE_HIP(c, hipSetDevice(c->device));
    PCE_HIP(c, c->si_pl.reserve(sizeof(unsigned long long) * (size_t)(p_off + 1)));
    PCE_HIP(c, c->si_csum.reserve(sizeof(unsigned long long) * (size_t)(chunk_off + 1)));
    PCE_HIP(c, c->si_coff.reserve(sizeof(unsigned long long) * (size_t)(chunk_off + 1)));
    PCE_HIP(c, c->si_tsum.reserve(sizeof(SiTile) * (size_t)(tile_off + 1)));
    PCE_HIP(c, c->si_tin.reserve(sizeof(SiCarry) * (size_t)(tile_off + 1)));
    PCE_HIP(c, c->si_out.reserve(sizeof(int32_t) * 2 * (size_t)(range_off + 1)));
    PCE_UPLOAD(c, c->si_meta, meta);
    PCE_ZERO(int32_t, c, c->si_count, (size_t)(n + 1));
    const SiSlice *d_meta = c->si_meta.as<SiSlice>();
    if (chunk_off > 0) {
        const int lds_words = (int)chunk_words(1 << cb_log2);
        const size_t lds = (size_t)(lds_words + 16) * 4;
        const bool nt = c->clip_off.back() * 2 > ((int64_t)256 << 20);        // the batch does not fit the Infinity Cache
        {
            KernelTimer t(c, PCE_K_MS_ENERGY);
            auto launch = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3((unsigned)chunk_off), dim3(SI_THREADS), lds, c->stream, c->d_pcm, d_meta, (int)n, rk, ch, cb_log2, lds_words,
                                   c->si_pl.as<unsigned long long>(), c->si_csum.as<unsigned long long>());
            };
            if (nt) launch(k_ms_energy<true>); else launch(k_ms_energy<false>);
            PCE_HIP(c, hipGetLastError());
        }
        {
            KernelTimer t(c, PCE_K_SILENCE_SCAN);
            hipLaunchKernelGGL(k_silence_scan, dim3((unsigned)n), dim3(64), 0, c->stream, d_meta, c->si_csum.as<unsigned long long>(), c->si_coff.as<unsigned long long>());
            PCE_HIP(c, hipGetLastError());
        }
        auto tiles = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3((unsigned)tile_off), dim3(SI_THREADS), 0, c->stream, d_meta, (int)n, rk, ch, cb_log2, L, step, c->si_pl.as<unsigned long long>(),
                               c->si_coff.as<unsigned long long>(), c->si_tsum.as<SiTile>(), c->si_tin.as<SiCarry>(), c->si_out.as<int>());
        };
        { KernelTimer t(c, PCE_K_SILENCE_RANGES); tiles(k_silence_ranges<false>); PCE_HIP(c, hipGetLastError()); }
        {
            KernelTimer t(c, PCE_K_SILENCE_RANGES);
            hipLaunchKernelGGL(k_silence_carry, dim3((unsigned)n), dim3(64), 0, c->stream, d_meta, L, step, c->si_tsum.as<SiTile>(), c->si_tin.as<SiCarry>(), c->si_out.as<int>(),
                               c->si_count.as<int>());
            PCE_HIP(c, hipGetLastError());
        }
        { KernelTimer t(c, PCE_K_SILENCE_RANGES); tiles(k_silence_ranges<true>); PCE_HIP(c, hipGetLastError()); }
    }
    PCE_HIP(c, hipStreamSynchronize(c->stream));                 // `meta` is pageable and dies at return
    c->si_counts_valid = false;
    c->si_n = n;
    return PCE_OK;
}

static int si_counts(pce_ctx *c)
{
    if (c->si_counts_valid) return PCE_OK;
    c->si_counts.assign((size_t)c->si_n + 1, 0);
    PCE_HIP(c, hipSetDevice(c->device));
    if (c->si_n > 0)
        PCE_FETCH(c, c->si_counts.data(), c->si_count.p, (size_t)c->si_n);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    pce_profile_collect(c);
    for (int32_t i = 0; i < c->si_n; i++) {
        const int64_t cap = c->si_cap_off[(size_t)i + 1] - c->si_cap_off[(size_t)i];
        if (c->si_counts[(size_t)i] < 0 || c->si_counts[(size_t)i] > cap)
            return pce_fail(c, PCE_E_DEVICE, "silence: slice %d reports %d ranges, the bound is %lld", i, c->si_counts[(size_t)i], (long long)cap);
    }
    c->si_counts_valid = true;
    return PCE_OK;
}

int pce_silence_shape(pce_ctx *c, int64_t *range_offsets, int32_t *len_ms, int32_t *status)
{
    if (!c || !range_offsets) return PCE_E_INVALID;
    if (c->si_n < 0) return pce_fail(c, PCE_E_STATE, "pce_silence_shape before pce_silence_run");
    PCE_TRY(si_counts(c));
    range_offsets[0] = 0;
    for (int32_t i = 0; i < c->si_n; i++) {
        range_offsets[i + 1] = range_offsets[i] + c->si_counts[(size_t)i];
        if (len_ms) len_ms[i] = c->si_len_ms[(size_t)i];
        if (status) status[i] = c->si_status[(size_t)i];
    }
    return PCE_OK;
}

int pce_silence_fetch(pce_ctx *c, int32_t *ranges)
{
    if (!c) return PCE_E_INVALID;
    if (c->si_n < 0) return pce_fail(c, PCE_E_STATE, "pce_silence_fetch before pce_silence_run");
    PCE_TRY(si_counts(c));
    const int64_t cap_total = c->si_cap_off[(size_t)c->si_n];
    int64_t total = 0;
    for (int32_t i = 0; i < c->si_n; i++) total += c->si_counts[(size_t)i];
    if (total == 0) return PCE_OK;
    if (!ranges) return PCE_E_INVALID;
    std::vector<int32_t> all((size_t)cap_total * 2);
    PCE_FETCH(c, all.data(), c->si_out.p, 2 * (size_t)cap_total);
    PCE_HIP(c, hipStreamSynchronize(c->stream));
    int64_t w = 0;
    for (int32_t i = 0; i < c->si_n; i++) {
        const size_t cnt = (size_t)c->si_counts[(size_t)i];
        if (cnt) memcpy(ranges + 2 * w, all.data() + 2 * (size_t)c->si_cap_off[(size_t)i], sizeof(int32_t) * 2 * cnt);
        w += (int64_t)cnt;
    }
    return PCE_OK;
}

} // extern "C"
