// pce_decode_kernels.inc -- the text decoder's own kernels: token embedding, K / V cache writes, the single-query attention kernels of an incremental
// step (k_cross_attn1w, k_self_attn1w) and their launchers (included by pce_whisper_impl.inc inside its anonymous namespace).
// ---------------------------------------------------------------------------
// Text decoder (teacher forced) and cross-attention alignment  -- openai-whisper timing.py find_alignment
// ---------------------------------------------------------------------------
__global__ void k_embed_tokens(const int *__restrict__ tokens /* [clips][T_pad] */, const float *__restrict__ tok_emb,
                               const float *__restrict__ pos_emb, int T_pad, int n_ctx, int d, int64_t rows, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * d) return;
    const int64_t m = i / d; const int col = (int)(i - m * d);
    int t = (int)(m % T_pad); if (t >= n_ctx) t = n_ctx - 1;      // pad rows beyond the clip's tokens: any finite value
    out[i] = tok_emb[(int64_t)tokens[m] * d + col] + pos_emb[(int64_t)t * d + col];
}

// last position of every sequence: resid row (clip * T_pad + len - 1) -> out row clip
__global__ void k_gather_last(const float *__restrict__ resid, const int *__restrict__ t_len, int T_pad, int d, int n, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * d) return;
    const int clip = (int)(i / d), col = (int)(i - (int64_t)clip * d);
    out[i] = resid[((int64_t)clip * T_pad + t_len[clip] - 1) * d + col];
}

// self-attention cache maintenance.  k_cache_k: K rows of a prefix run, [clip * T_pad + t][2d] (second half) -> cache
// [clip][T_cap][d] (an incremental step's attention kernel appends its new position itself).
__global__ void k_cache_k(const op_t *__restrict__ qk, int T_pad, const int *__restrict__ t_len, int d, int T_cap, int n, op_t *__restrict__ ck)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * T_pad * d) return;
    const int col = (int)(i % d); const int64_t r = i / d; const int t = (int)(r % T_pad), clip = (int)(r / T_pad);
    if (t < t_len[clip]) ck[((int64_t)clip * T_cap + t) * d + col] = qk[r * 2 * d + d + col];
}
// V rows of a prefix run for the incremental steps' self-attention: V^T image [clip][d][sp] (written by the QKV epilogue) -> row-major [clip][T_cap][d]
__global__ void k_cache_v_rows(const op_t *__restrict__ cvt, const int *__restrict__ t_len, int d, int T_cap, int sp, int n, op_t *__restrict__ cv)
{
    __shared__ op_t t[32][33];
    const int clip = blockIdx.z, c0 = blockIdx.x * 32, t0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int T = t_len[clip];
    if (t0 >= T) return;
    for (int r = ty; r < 32; r += 8) t[r][tx] = cvt[((int64_t)clip * d + c0 + r) * sp + t0 + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (t0 + r < T) cv[((int64_t)clip * T_cap + t0 + r) * d + c0 + tx] = t[tx][r];
}

// Self-attention of an incremental decoding step on ROW-MAJOR caches (K rows and V rows [clip][T_cap][d]): one wave per (clip, head), one
// workgroup per clip.  Appending the new position is two coalesced 128-byte row stores per wave -- the V^T image of the prefix kernels would take
// 64 two-byte stores at a 1 KB stride, which was a third of this launch (profiles/r05/xattn_absorb.txt).  Scores as k_cross_attn1w computes them
// (8 lanes per key row, eight rows per lane in flight, fp32 softmax in LDS); the weighted sum over V walks the rows the same way, every lane
// accumulating its 8 dimensions over the keys of its group, the eight groups added by shuffles.  The new key / value are attended to from registers.
struct SelfAttn1Args {
    const op_t *qkv; int64_t qkv_ld;          // the new position: q | k | v of clip c at qkv + c * qkv_ld (+ d, + 2 d)
    op_t *ck, *cv; int64_t c_clip; int d;     // caches: row t of clip c at + c * c_clip + t * d
    const int *pos, *skip;                    // position of the new token (= cached keys) per clip; skip may be null
    op_t *out; int64_t out_ld;
    int heads;
};
// More than 16 heads (large-v3 / turbo: 20): the heads are cut into groups of at most 16 waves, one workgroup per (clip, group) -- grid (clips, groups),
// wave w of group y is head y * (waves per group) + w; each wave appends its own head's columns.  Up to 16 heads: one group, the launch of round 5.
__global__ __launch_bounds__(1024) void k_self_attn1w(SelfAttn1Args A)
{
    extern __shared__ float sa_sp[];                              // [waves of the group][512]
    const int clip = blockIdx.x;
    if (A.skip && A.skip[clip]) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = (int)blockIdx.y * (int)(blockDim.x >> 6) + wv;
    if (head >= A.heads) return;                                  // (a short last group; no barrier in this kernel)
    float *sp = sa_sp + wv * 512;
    const int Sc = A.pos[clip];                                   // cached keys 0 .. Sc - 1; the new one is key Sc
    const int g = lane >> 3, ch = lane & 7;
    const op_t *nq = A.qkv + (int64_t)clip * A.qkv_ld + head * 64;
    const opx8 qv = *reinterpret_cast<const opx8 *>(nq + ch * 8);
    const opx8 k_new = *reinterpret_cast<const opx8 *>(nq + A.d + ch * 8), v_new = *reinterpret_cast<const opx8 *>(nq + 2 * A.d + ch * 8);
    const op_t kn = nq[A.d + lane], vn = nq[2 * A.d + lane];
    op_t *ckb = A.ck + (int64_t)clip * A.c_clip + head * 64, *cvb = A.cv + (int64_t)clip * A.c_clip + head * 64;
    ckb[(int64_t)Sc * A.d + lane] = kn;                           // (nothing in this launch reads row Sc back)
    cvb[(int64_t)Sc * A.d + lane] = vn;
    float qf[8];
#pragma unroll
    for (int e = 0; e < 8; e++) qf[e] = (float)qv[e] * 0.125f;
    constexpr int U = 8;
    float m = -3.0e38f;
    for (int base = 0; base < Sc; base += 8 * U) {
        opx8 kv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = base + u * 8 + g;
            kv[u] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(ckb + (int64_t)(r < Sc ? r : Sc - 1) * A.d + ch * 8));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            float dd = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) dd = fmaf((float)kv[u][e], qf[e], dd);
            dd += __shfl_xor(dd, 1, 64); dd += __shfl_xor(dd, 2, 64); dd += __shfl_xor(dd, 4, 64);
            const int r = base + u * 8 + g;
            if (r < Sc) { m = fmaxf(m, dd); if (ch == 0) sp[r] = dd; }
        }
    }
    float s_new;
    {
        float dd = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) dd = fmaf((float)k_new[e], qf[e], dd);
        dd += __shfl_xor(dd, 1, 64); dd += __shfl_xor(dd, 2, 64); dd += __shfl_xor(dd, 4, 64);
        s_new = dd; m = fmaxf(m, dd);
    }
    m = wave_xor_max(m);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    float sum = 0.f;
    for (int t = lane; t < Sc; t += 64) {
        const float pv = __expf(sp[t] - m);
        sp[t] = pv; sum += pv;
    }
    sum = wave_xor_sum(sum);
    const float p_new = __expf(s_new - m);                       // (the same value in every lane)
    sum += p_new;
    const float inv = 1.0f / sum;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] = 0.f;
    for (int base = 0; base < Sc; base += 8 * U) {
        opx8 vv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = base + u * 8 + g;
            vv[u] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(cvb + (int64_t)(r < Sc ? r : Sc - 1) * A.d + ch * 8));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = base + u * 8 + g;
            const float wgt = r < Sc ? sp[r] : 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) acc[e] = fmaf(wgt, (float)vv[u][e], acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
        float a = acc[e];
        a += __shfl_xor(a, 8, 64); a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
        acc[e] = fmaf(p_new, (float)v_new[e], a) * inv;
    }
    if (g == 0) {
        opx8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (op_t)acc[e];
        *reinterpret_cast<opx8 *>(A.out + (int64_t)clip * A.out_ld + head * 64 + ch * 8) = o;
    }
}
__global__ void k_embed_one(const int *__restrict__ tok, const float *__restrict__ tok_emb, const float *__restrict__ pos_emb,
                            const int *__restrict__ pos_of, int d, int n, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * d) return;
    const int clip = (int)(i / d), col = (int)(i - (int64_t)clip * d);
    out[i] = tok_emb[(int64_t)tok[clip] * d + col] + pos_emb[(int64_t)pos_of[clip] * d + col];
}

// ---- device-resident decoding loop (round 3) -----------------------------------------------------------------------------------
// After the logit filters have chosen `next` for every sequence, k_step_advance appends it to the device-resident token table,
// refreshes the per-sequence tables the NEXT step's kernels read (new token, position, self-attention key count, "ended" flag),
// records the step's outputs and counts the sequences whose last token is end-of-text.  Nothing of a step passes through the host.
// tables ct[8 n]: new token | q_row0 | q_len | k_row0 | k_len | a_row0 | a_len | position   (the layout pce_whisper_decode_step_ex uploads)
__global__ __launch_bounds__(256) void k_step_advance(int n, int T_cap, int eot, int max_new, int *__restrict__ tok_table, int *__restrict__ len,
                                                     const int *__restrict__ next, const float *__restrict__ next_lp, int *__restrict__ ct,
                                                     int *__restrict__ ended, int *__restrict__ out_tok, float *__restrict__ out_lp,
                                                     int *__restrict__ step_ctr, int *__restrict__ n_ended)
{   // ONE workgroup (a few hundred sequences)
    const int step = *step_ctr;
    __syncthreads();
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int L = len[i], t = next[i];
        if (step < max_new) { out_tok[(size_t)i * max_new + step] = t; out_lp[(size_t)i * max_new + step] = next_lp[i]; }
        // L == T_cap: `t` followed a forward pass over the FULL text context; it is reported (out_tok above) but cannot be fed back.  The
        // sequence stops here, the reference's `tokens.shape[-1] > n_ctx: break`: the last table entry becomes end-of-text so that every later
        // step reads the sequence as ended (its real value has already left through out_tok one step earlier).
        if (L < T_cap) { tok_table[(size_t)i * T_cap + L] = t; len[i] = L + 1; }
        else tok_table[(size_t)i * T_cap + T_cap - 1] = eot;
        ct[i] = t; ct[4 * n + i] = (L < T_cap ? L : T_cap - 1) + 1; ct[7 * n + i] = L < T_cap ? L : T_cap - 1;
        const int e = t == eot || L >= T_cap;
        ended[i] = e; cnt += e;
    }
    if (cnt) atomicAdd(n_ended + (step < max_new ? step : max_new - 1), cnt);
    if (threadIdx.x == 0) *step_ctr = step + 1;
}

// Attention of ONE query per (clip, head) over a long key axis: the cross-attention (1 500 audio positions) and the cached
// self-attention of an incremental decoding step.  The MFMA attention kernels spend a 32-query tile on it and walk the keys as 24
// dependent LDS-DMA tiles per workgroup; this is a streaming kernel: HBM-bound by construction (one pass over K, one over V^T:
// 14 GB per step for 256 clips at Whisper-small size, the roofline of free-running decoding).
//   phase 1: scores.  8 lanes per key row (16 B = 8 dims each: a wave-instruction covers eight whole 128-byte lines), eight rows per lane
//            in flight, 8-lane sums by DPP -> fp32 scores in LDS
//   phase 2: softmax (fp32, max-subtracted) in LDS
//   phase 3: O[d] = sum_t p[t] V^T[d][t]: the wave streams the V^T rows of its head as 1 KB pieces (lane = 8 consecutive keys, p in registers)
// `skip[clip]` != 0: the sequence has ended, its output is never used (the filters return end-of-text for it): no bytes are read.
struct Attn1Args {
    const op_t *q; int64_t q_ld;              // query of clip c: q + c * q_ld + head * 64
    const op_t *k; int64_t k_ld;              // key row j:       k + (k_row0[c] + j) * k_ld + head * 64
    const op_t *vt; int64_t vt_clip; int vt_sp;   // V^T:        vt + c * vt_clip + (head * 64 + d) * vt_sp + j   (columns >= k_len hold finite values)
    const int *k_row0, *k_len;                // per clip; k_len <= 1536
    const int *skip;                          // per clip or null
    op_t *out; int64_t out_ld;                // out + c * out_ld + head * 64
    // when app_pos is set, the wave of (clip, head) first writes the new position's key / value slice (app_k / app_v + c * app_ld + head * 64)
    // into K row app_pos[c] and V^T column app_pos[c], then attends
    const op_t *app_k, *app_v; int64_t app_ld; const int *app_pos;
    int heads;                                // heads in all (the grid's y counts head groups)
};
// k_cross_attn1w: ONE WAVE per (clip, head) and one workgroup per clip (wave = head).  Why: a key row is the
// 128-byte slices of all heads side by side (1 536 B at Whisper-small size); with a workgroup per (clip, head) the twelve slices of a row
// are fetched by twelve workgroups on different XCDs at different times -- twelve visits to the same DRAM page; here the waves of a
// workgroup walk the rows together.  Each wave keeps its scores in its own LDS slice: no workgroup barrier anywhere.
// More than 16 heads: groups of at most 16 waves, grid (clips, groups), as k_self_attn1w.
__global__ __launch_bounds__(1024) void k_cross_attn1w(Attn1Args A)
{
    extern __shared__ float spw[];                               // [waves of the group][1536 + 64]
    const int clip = blockIdx.x;
    if (A.skip && A.skip[clip]) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = (int)blockIdx.y * (int)(blockDim.x >> 6) + wv;
    if (head >= A.heads) return;                                  // (a short last group)
    float *sp = spw + wv * 1600;
    const int Sk = A.k_len[clip];
    const int g = lane >> 3, ch = lane & 7;
    // Appending (the self-attention of an incremental step): the new position's key and value go to the cache with plain stores that
    // nothing in this launch reads back -- the wave attends to the new key from registers (its score from the key slice it has just
    // loaded, its value added after the sums over the cached keys), so there is no store -> wait -> load chain (that chain cost as much
    // as the separate append launch it replaced: 7 us).  The V^T cache only ever holds finite values (zeroed at allocation).
    const bool app = A.app_pos != nullptr;
    const int pos = app ? A.app_pos[clip] : 0;                    // == Sk - 1 when appending
    const int Sc = app ? Sk - 1 : Sk;                             // keys read from memory
    float v_new = 0.f;
    opx8 k_new;
#pragma unroll
    for (int e = 0; e < 8; e++) k_new[e] = (op_t)0.f;
    if (app) {
        const op_t kn = A.app_k[(int64_t)clip * A.app_ld + head * 64 + lane], vn = A.app_v[(int64_t)clip * A.app_ld + head * 64 + lane];
        const_cast<op_t *>(A.k)[((int64_t)A.k_row0[clip] + pos) * A.k_ld + head * 64 + lane] = kn;
        const_cast<op_t *>(A.vt)[(int64_t)clip * A.vt_clip + (int64_t)(head * 64 + lane) * A.vt_sp + pos] = vn;
        v_new = (float)vn;
        k_new = *reinterpret_cast<const opx8 *>(A.app_k + (int64_t)clip * A.app_ld + head * 64 + ch * 8);
    }
    float qf[8];
    {
        const opx8 qv = *reinterpret_cast<const opx8 *>(A.q + (int64_t)clip * A.q_ld + head * 64 + ch * 8);
#pragma unroll
        for (int e = 0; e < 8; e++) qf[e] = (float)qv[e] * 0.125f;
    }
    const op_t *kb = A.k + (int64_t)A.k_row0[clip] * A.k_ld + head * 64 + ch * 8;
    constexpr int U = 8;
    float m = -3.0e38f;
    for (int base = 0; base < Sc; base += 8 * U) {
        opx8 kv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = base + u * 8 + g;
            kv[u] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(kb + (int64_t)(r < Sc ? r : Sc - 1) * A.k_ld));
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < 8; e++) d = fmaf((float)kv[u][e], qf[e], d);
            d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
            const int r = base + u * 8 + g;
            if (r < Sc) { m = fmaxf(m, d); if (ch == 0) sp[r] = d; }
        }
    }
    if (app) {                                                    // the new key, scored the same way (same operation order as a cached row)
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < 8; e++) d = fmaf((float)k_new[e], qf[e], d);
        d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
        m = fmaxf(m, d);
        if (lane == 0) sp[pos] = d;
    }
    m = wave_xor_max(m);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    float sum = 0.f;
    const int Sp = (Sk + 511) & ~511;
    for (int t = lane; t < Sp; t += 64) {
        const float pv = t < Sk ? __expf(sp[t] - m) : 0.f;
        sp[t] = pv; sum += pv;
    }
    sum = wave_xor_sum(sum);
    const float inv = 1.0f / sum;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
    const int np = Sp >> 9;
    const float p_new = app ? sp[pos] : 0.f;                     // weight of the new key
    if (Sk <= 128) {
        // few keys (the self-attention of a decoding step): lane d owns output dimension d and reads the first Sk keys of ITS V^T row, all
        // sixteen 16-byte loads requested at once -- one memory round trip.  (The general form below walks the 64 rows four at a time:
        // sixteen dependent round trips, 42-51 us per launch for a few dozen keys.)
        const op_t *vr = A.vt + (int64_t)clip * A.vt_clip + (int64_t)(head * 64 + lane) * A.vt_sp;
        opx8 vv[16];
#pragma unroll
        for (int cc = 0; cc < 16; cc++) {
#pragma unroll
            for (int e = 0; e < 8; e++) vv[cc][e] = (op_t)0.f;
            if (cc * 8 < Sk) vv[cc] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(vr + cc * 8));
        }
        float a = 0.f;
#pragma unroll
        for (int cc = 0; cc < 16; cc++)
            if (cc * 8 < Sk) {                                   // (wave-uniform)
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const int t = cc * 8 + e;
                    const float wgt = (app && t == pos) ? 0.f : sp[t];      // (column `pos` is being written by this very launch: weight 0; sp[t] = 0 beyond the last key)
                    a = fmaf(wgt, (float)vv[cc][e], a);
                }
            }
        if (app) a = fmaf(p_new, v_new, a);
        A.out[(int64_t)clip * A.out_ld + head * 64 + lane] = (op_t)(a * inv);
        return;
    }
    float pr[3][8];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int t = j * 512 + lane * 8 + e;
            pr[j][e] = (j < np && !(app && t == pos)) ? sp[t] : 0.f;     // (the cached column `pos` is being written by this very launch: weight 0)
        }
    const op_t *vb = A.vt + (int64_t)clip * A.vt_clip + (int64_t)(head * 64) * A.vt_sp + lane * 8;
    const int v_new_bits = __builtin_bit_cast(int, v_new);
    float keep = 0.f;                                            // lane d ends up with output dimension d
#pragma unroll 2
    for (int r4 = 0; r4 < 64; r4 += 4) {
        // a lane whose eight keys all lie beyond the last key does not load (its weights are zero): the self-attention of a decoding step
        // has a few dozen keys in a 512-column image -- reading whole rows cost 200 MB and ~50 us per launch for 20 MB of live values
        opx8 vv[4][3];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
#pragma unroll
                for (int e = 0; e < 8; e++) vv[r][j][e] = (op_t)0.f;
                if (j < np && j * 512 + lane * 8 < Sk) vv[r][j] = __builtin_nontemporal_load(reinterpret_cast<const opx8 *>(vb + (int64_t)(r4 + r) * A.vt_sp + j * 512));
            }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (j < np)
#pragma unroll
                    for (int e = 0; e < 8; e++) a = fmaf(pr[j][e], (float)vv[r][j][e], a);
            a = wave_xor_sum(a);
            if (app) a = fmaf(p_new, __builtin_bit_cast(float, __builtin_amdgcn_readlane(v_new_bits, r4 + r)), a);
            if (lane == r4 + r) keep = a * inv;
        }
    }
    A.out[(int64_t)clip * A.out_ld + head * 64 + lane] = (op_t)keep;
}

// The launches of the two single-query kernels, n clips x H heads (the decoding step and pce_selftest_attn1 make them here).  Up to 16 heads: one
// workgroup per clip, one wave per head (115.8 against 119.6 us per launch with a workgroup per clip and head).  More heads (20 at large-v3 /
// turbo): workgroups of at most 16 waves, grid (clip, head group) -- lds_optins (16 waves' slices) covers the largest group.
static void launch_cross_attn1(pce_ctx *c, int n, int H, const Attn1Args &args)
{
    const int hgroups = (H + 15) / 16, hg_waves = (H + hgroups - 1) / hgroups;
    Attn1Args a = args;
    a.heads = H;
    KernelTimer kt(c, PCE_K_CROSS_ATTN1);
    hipLaunchKernelGGL(k_cross_attn1w, dim3((unsigned)n, (unsigned)hgroups), dim3(64 * (unsigned)hg_waves), (size_t)hg_waves * 1600 * 4, c->stream, a);
}
static void launch_self_attn1(pce_ctx *c, int n, int H, const SelfAttn1Args &args)
{
    const int hgroups = (H + 15) / 16, hg_waves = (H + hgroups - 1) / hgroups;
    SelfAttn1Args a = args;
    a.heads = H;
    KernelTimer kt(c, PCE_K_CROSS_ATTN1);
    hipLaunchKernelGGL(k_self_attn1w, dim3((unsigned)n, (unsigned)hgroups), dim3(64 * (unsigned)hg_waves), (size_t)hg_waves * 512 * 4, c->stream, a);
}
