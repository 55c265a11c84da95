// pce_xattn.inc -- cross-attention of an incremental decoding step computed from the ENCODER OUTPUT instead of from projected keys / values
// (round 5; included by pce_whisper_impl.inc inside its anonymous namespace, compiled once per operand type).
//
// openai-whisper's MultiHeadAttention (model.py: k = key(xa), v = value(xa), softmax(q k^T / sqrt(64)) v, `key` without bias) for ONE query
// position per clip.  With E = xa (the encoder output, [1500][d]) and the per-head slices Wk_h, Wv_h ([64][d]):
//     scores_h[t] = q_h . (Wk_h E[t])            = (q_h Wk_h) . E[t]            = Q'_h . E[t]          Q' = [heads][d]
//     out_h       = sum_t p_h[t] (Wv_h E[t] + bv_h) = Wv_h (sum_t p_h[t] E[t]) + bv_h = Wv_h U_h + bv_h     U  = [heads][d]
// The streaming kernel of round 3 (k_cross_attn1w) reads the projected K rows and V^T of every layer -- 2 x 1500 x d x 2 B per clip and layer,
// 14.3 GB per step for 256 clips at Whisper-small size: the roofline of free-running decoding.  This form reads E ONCE per layer (7.1 GB):
// half the HBM bytes of the kernel that was 72 % of a step, for 12 x the -- still negligible -- matrix work (all heads share E, so the
// products are 16-row MFMA tiles: the heads are the rows).  Three launches per layer:
//   k_xq_fused         q = Wq ln + bq (rounded to op_t), Q'[clip][h][:] = (log2 e / 8) q_h Wk_h   (Wk^T built at load time)
//   k_xattn_absorbed   one pass over E: S^T = E Q'^T, online softmax, U^T = E^T P^T; (clip, split of the frames) per workgroup
//   k_uv_absorb        merges the splits, out_h = Wv_h U_h + bv_h
// Arithmetic: Q', P and U enter their MFMAs as hi + lo pairs of op_t (two products each), so the rounding the reference's own arithmetic has
// at k = key(xa) / v = value(xa) / softmax(...).to(fp16) is not replaced by a coarser one: against the fp32 restatement this path is as close as
// the K / V path (tests/test_gpu_whisper.py compares both with it, step by step; the prefix step of a decode still runs on the K / V cache).
// tests/test_gpu_xattn.py holds each of the three kernels to that claim on its own (pce_selftest_xattn_stages copies out Q', the nodes' U and (m, l)).
// profiles/r05/xattn_absorb.txt: the development bench (tools/lab/xattn_absorb.hip) and the A/B of the decoding loop.

typedef short xa_s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
typedef __attribute__((ext_vector_type(4))) op_t xa_opx4;

template <class T> struct XaMfmaK16;
template <> struct XaMfmaK16<_Float16> {
    static __device__ __forceinline__ f32x4 run(xa_s16x4 a, xa_opx4 b, f32x4 c)
    {
        typedef __attribute__((ext_vector_type(4))) _Float16 h4;
        return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h4, a), __builtin_bit_cast(h4, b), c, 0, 0, 0);
    }
};
template <> struct XaMfmaK16<__bf16> {
    static __device__ __forceinline__ f32x4 run(xa_s16x4 a, xa_opx4 b, f32x4 c)
    {
        typedef __attribute__((ext_vector_type(4))) short s4;
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4, a), __builtin_bit_cast(s4, b), c, 0, 0, 0);
    }
};

// LDS image of a 16-frame tile of E: the rows as they lie in memory (row pitch 2 d bytes, a multiple of 256), the sixteen 16-byte chunks of every
// 256-byte group XOR-swizzled by the row (cdna_hip_programming.md T10, image (b)): it serves the row reads of S^T = E Q'^T and the transposed
// reads (ds_read_b64_tr_b16) of U^T = E^T P^T, and a DMA instruction (64 consecutive chunks of the image) still reads 1 KB of contiguous memory.
__device__ __forceinline__ int xa_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
template <int D> __device__ __forceinline__ int xa_off(int row, int col8 /* 16-byte chunk of the row: column / 8 */) { return 2 * D * row + 16 * (col8 ^ xa_swz(row)); }
// (through asm: the builtin makes the compiler wait for ALL outstanding LDS-DMA -- vmcnt(0) -- before the read, which drains the ring every tile)
__device__ __forceinline__ xa_s16x4 xa_tr_read(unsigned addr) { xa_s16x4 r; asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr)); return r; }

struct XaArgs {
    const op_t *E; int64_t e_clip; int e_ld;        // E + clip * e_clip + t * e_ld (+ column)
    const op_t *qp_hi, *qp_lo;                      // [clip][R][D]: Q' (scaled by log2 e / sqrt(head size)); rows >= heads are never used
    const int *k_len, *skip;                        // per clip; skip may be null
    float *u_part;                                  // [clip][nodes][R][D]: sum_t 2^(s_t - m) E[t] over the frames of one node (nodes = 4 leaves, or 2 pairs: PAIR kernels)
    float *ml_part;                                 // [clip][nodes][R][2]: the node's reference m and sum l
    int heads, nsplit;                              // nsplit: workgroups per clip (1, 2 or 4); each walks XA_LEAVES / nsplit consecutive leaves
    int rows;                                       // R = 16 ceil(heads / 16): the heads are the rows of R / 16 MFMA row tiles (16 up to 16 heads, 32 at 20)
};
constexpr int xa_rows(int heads) { return 16 * ((heads + 15) / 16); }

// The frames of a clip are ALWAYS cut into the same four LEAVES, each with its own online softmax, and the leaves are ALWAYS combined in the same tree
// (L0 + L1) + (L2 + L3), "+" = xa_merge below -- whatever the batch size.  Round 5 cut the frames into as many ranges as workgroups per clip (8 / 4 / 2 / 1 by
// batch size) and merged them flat: a clip's cross-attention bits, and now and then a token, followed from how many clips shared its batch (ADVICE r05;
// include/pce.h promises the opposite since minor 2).  Now only the NUMBER OF WORKGROUPS follows the batch size.  A workgroup that owns several leaves streams
// through them in one ring and starts a fresh (m, l, U) at every leaf boundary; one that owns both leaves of a PAIR combines them in registers (the first
// leaf's U waits in 48 more VGPRs at d = 768) and writes the pair's node, so that 256 clips exchange two partials per clip as round 5 did -- four leaves
// written and read back cost 2.50 ms per incremental step against round 5's 2.33, eight leaves 2.73 (same box, profiles/r06/xattn_leaves_ab.txt).
// k_uv_absorb finishes the tree from whichever nodes it is handed: the same operations in the same order as the in-register form, the same bits.
#ifndef PCE_XA_LEAVES
#define PCE_XA_LEAVES 4
#endif
constexpr int XA_TF = 16, XA_LEAVES = PCE_XA_LEAVES, XA_MAX_SPLIT = XA_LEAVES;
static_assert(XA_LEAVES == 4, "the merge tree of k_uv_absorb is written for four leaves");
// node a + node b of the merge tree: reference m = max, both sides rescaled by exact-or-rounded powers of two, l and every element of U by ONE fma
__device__ __forceinline__ void xa_merge_w(float ma, float mb, float &m, float &wa, float &wb)
{
    m = fmaxf(ma, mb); wa = __builtin_amdgcn_exp2f(ma - m); wb = __builtin_amdgcn_exp2f(mb - m);
}
__device__ __forceinline__ float xa_merge_v(float a, float wa, float b, float wb) { return fmaf(b, wb, a * wa); }

// one workgroup = one (clip, split), WV waves: wave w owns d / WV of the reduction axis of S^T (partials summed through LDS, every wave in the same
// order: the same bits) and d / WV of the columns of U^T.  E streams through a ring of NSLOT slots by LDS-DMA with the non-temporal policy (it is read
// once per launch and is larger than every cache: without `nt` the same instruction stream is 14 % slower, tools/lab/xattn_absorb.hip).
// d <= 1024 (at most 16 heads): 4 waves, one row tile of heads, two or three workgroups per CU.  d = 1280 (20 heads: large-v3 / turbo): 8 waves and
// RT = 2 row tiles (rows 16..31 hold heads 16..19 and unused rows): the 4-wave body would hold 160 Q' and 160 U registers per wave at two row tiles;
// with 8 waves each wave keeps 5 k-steps x 2 tiles of Q' (hi + lo: 80 VGPRs) and 10 column blocks x 2 tiles of U (80), and E still streams once
// per layer -- every column block of E^T serves both row tiles.  One workgroup per CU (three 40 KB slots + 16 KB of partials), two waves per SIMD.
template <int D, int NSLOT, bool PAIR, int WV, int RT>
__device__ __forceinline__ void xattn_absorbed_body(const XaArgs &A, char *smem)
{
    static_assert(D % (32 * WV) == 0 && (RT == 1 || !PAIR), "a wave owns whole k-steps; the in-register pair form holds one row tile");
    constexpr int TF = XA_TF, KS = D / (32 * WV), CB = D / (16 * WV), LPW = D / (32 * WV), TILE = TF * D * 2;   // k-steps / column blocks / DMA instructions per wave; tile bytes
    const int bid = (int)blockIdx.x;
    const int clip = bid / A.nsplit, split = bid - clip * A.nsplit;
    if (A.skip && A.skip[clip]) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n16 = lane & 15, g = lane >> 4;
    const int Sk = A.k_len[clip];
    const int nt_all = (Sk + TF - 1) / TF, per = (nt_all + XA_LEAVES - 1) / XA_LEAVES;      // tiles per leaf: a function of the clip alone
    const int lpw = XA_LEAVES / A.nsplit, leaf0 = split * lpw;                              // this workgroup's leaves: leaf0 .. leaf0 + lpw - 1
    const int t_lo = leaf0 * per, nt = max(min(nt_all, t_lo + lpw * per) - t_lo, 0);
    const op_t *eb = A.E + (int64_t)clip * A.e_clip;
    const __amdgpu_buffer_rsrc_t rsE = __builtin_amdgcn_make_buffer_rsrc(const_cast<op_t *>(eb), 0, ((Sk - 1) * A.e_ld + D) * 2, 0x00020000);
    // Q' fragments of this wave's slice of the d axis (B operand: lane (n16 = head row of row tile rt, g) holds d = 32 kk + 8 g .. + 7)
    opx8 qh[RT][KS], ql[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const int64_t o = ((int64_t)clip * A.rows + 16 * rt + n16) * D + 32 * (wv * KS + ks) + 8 * g;
            qh[rt][ks] = *reinterpret_cast<const opx8 *>(A.qp_hi + o);
            ql[rt][ks] = *reinterpret_cast<const opx8 *>(A.qp_lo + o);
        }
    // Q' must have ARRIVED before the ring starts: left to itself the compiler waits for these loads at their first use inside the loop with a
    // vmcnt count that also drains the tile prefetched behind them -- every iteration
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ks = 0; ks < KS; ks++) asm volatile("s_waitcnt vmcnt(0)" : "+v"(qh[rt][ks]), "+v"(ql[rt][ks]));
    int voff[LPW];
#pragma unroll
    for (int i = 0; i < LPW; i++) {
        const int X = 64 * (wv + WV * i) + lane, row = X / (D / 8), ch = (X % (D / 8)) ^ xa_swz(row);
        voff[i] = (row * A.e_ld + 8 * ch) * 2;
    }
    auto stage = [&](int t) {
        char *slot = smem + (t % NSLOT) * TILE;
#pragma unroll
        for (int i = 0; i < LPW; i++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsE, (__attribute__((address_space(3))) void *)(slot + 1024 * (wv + WV * i)), 16, voff[i], (t_lo + t) * TF * A.e_ld * 2, 0, 3 /* sc0 | nt: streamed once, see the header */);
    };
    int raddr[KS];                                               // row reads: frame pi(n16), d chunk of k-step wv KS + ks
    // The 16 frames of a tile sit on the MFMA rows in the order pi(m) = 4 sigma(m >> 2) + (m & 3), sigma = (0, 2, 1, 3): lane group g then holds the scores of
    // frames 4 sigma(g) .. + 3, and the transposed reads of a 32-lane half take two blocks 8 rows apart (conflict-free) instead of two stacked in one
    // 8-row group (2-way, cdna_hip_programming.md T10).  The softmax does not care about the order of the frames.
    const int sg = ((g & 1) << 1) | (g >> 1);                    // sigma(g)
    const int pr = 4 * (((n16 >> 2) & 1) << 1 | (n16 >> 3)) + (n16 & 3);   // pi(n16)
#pragma unroll
    for (int ks = 0; ks < KS; ks++) raddr[ks] = xa_off<D>(pr, 4 * (wv * KS + ks) + g);
    const int q4 = n16 >> 2, p4 = n16 & 3;
    float *xs = reinterpret_cast<float *>(smem + NSLOT * TILE);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 u[RT][CB];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int cb = 0; cb < CB; cb++) u[rt][cb] = z4;
    float m_run[RT], l_part[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) { m_run[rt] = -1e30f; l_part[rt] = 0.f; }
    // PAIR (a workgroup that owns both leaves of a pair): the even leaf's node waits here for the odd one
    f32x4 uh[PAIR ? CB : 1];
    float mh = -1e30f, lh = 0.f;
    auto flush = [&](int leaf) {                                 // a finished leaf: its node (U, reference m, sum l) leaves, or waits for / joins its pair
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            float l = l_part[rt];
            l += __shfl_xor(l, 16, 64);
            l += __shfl_xor(l, 32, 64);
            if (PAIR && !(leaf & 1)) {
#pragma unroll
                for (int cb = 0; cb < CB; cb++) uh[PAIR ? cb : 0] = u[0][cb];
                mh = m_run[0]; lh = l;
            } else {
                int node = leaf;
                float m_out = m_run[rt];
                if (PAIR) {                                      // (held even leaf) + (this odd leaf): xa_merge, as k_uv_absorb does it from stored leaves
                    float wa, wb;
                    xa_merge_w(mh, m_run[0], m_out, wa, wb);
                    l = xa_merge_v(lh, wa, l, wb);
#pragma unroll
                    for (int cb = 0; cb < CB; cb++)
#pragma unroll
                        for (int e = 0; e < 4; e++) u[0][cb][e] = xa_merge_v(uh[PAIR ? cb : 0][e], wa, u[0][cb][e], wb);
                    node = leaf >> 1;
                }
                constexpr int NODES = PAIR ? XA_LEAVES / 2 : XA_LEAVES;
                const int row = 16 * rt + n16;
                if (row < A.heads) {
                    float *up = A.u_part + (((int64_t)clip * NODES + node) * A.rows + row) * D;
#pragma unroll
                    for (int cb = 0; cb < CB; cb++) *reinterpret_cast<f32x4 *>(up + 16 * (wv * CB + cb) + 4 * g) = u[rt][cb];
                    if (wv == 0 && g == 0) { float *mp = A.ml_part + (((int64_t)clip * NODES + node) * A.rows + row) * 2; mp[0] = m_out; mp[1] = l; }
                }
            }
#pragma unroll
            for (int cb = 0; cb < CB; cb++) u[rt][cb] = z4;
            m_run[rt] = -1e30f; l_part[rt] = 0.f;
        }
    };
    int leaf = leaf0;
    for (int t = 0; t < NSLOT - 1 && t < nt; t++) stage(t);
    for (int t = 0; t < nt; t++) {
        if (NSLOT >= 3 && t + 1 < nt) __builtin_amdgcn_s_waitcnt(0x0F70 | ((NSLOT - 2) * LPW)); else __builtin_amdgcn_s_waitcnt(0x0F70 | 0);
        __builtin_amdgcn_s_barrier();                            // tile t has landed (every wave's part); everybody is done with tile t - 1
        if (t + NSLOT - 1 < nt) stage(t + NSLOT - 1);
        // (wave-uniform) tile t opens the next leaf: the finished one leaves HERE, behind the wait above -- vmcnt counts stores too, and a flush in front
        // of that wait made every leaf boundary sit out its own stores (26 us per launch at 256 clips); now they drain under this tile's MFMAs
        if (t > 0 && t - (leaf - leaf0 + 1) * per == 0) flush(leaf++);
        const char *sC = smem + (t % NSLOT) * TILE;
        const unsigned sbase = lds0 + (unsigned)((t % NSLOT) * TILE);
        {   // ---- partial S^T over this wave's share of d, every row tile
            f32x4 a[RT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) a[rt] = z4;
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                const opx8 ef = *reinterpret_cast<const opx8 *>(sC + raddr[ks]);
#pragma unroll
                for (int rt = 0; rt < RT; rt++) {
                    a[rt] = mfma16(ef, qh[rt][ks], a[rt]);
                    a[rt] = mfma16(ef, ql[rt][ks], a[rt]);
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; rt++) *reinterpret_cast<f32x4 *>(xs + ((wv * RT + rt) * 64 + lane) * 4) = a[rt];
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);                      // the partials are in LDS (lgkmcnt 0; the DMA of later tiles stays in flight)
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int f0 = (t_lo + t) * TF;
        xa_opx4 ph[RT], pl[RT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            f32x4 sc = z4;
#pragma unroll
            for (int w2 = 0; w2 < WV; w2++) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(xs + ((w2 * RT + rt) * 64 + lane) * 4);
                sc[0] += v[0]; sc[1] += v[1]; sc[2] += v[2]; sc[3] += v[3];
            }
            if (f0 + TF > Sk) {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (f0 + 4 * sg + i >= Sk) sc[i] = -1e30f;
            }
            float m = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            const float mx = fmaxf(m_run[rt], m);
            if (__builtin_amdgcn_ballot_w64(mx > m_run[rt]) != 0) {
                const float corr = __builtin_amdgcn_exp2f(m_run[rt] - mx);
                l_part[rt] *= corr;
#pragma unroll
                for (int cb = 0; cb < CB; cb++) { u[rt][cb][0] *= corr; u[rt][cb][1] *= corr; u[rt][cb][2] *= corr; u[rt][cb][3] *= corr; }
                m_run[rt] = mx;
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float pv = __builtin_amdgcn_exp2f(sc[i] - m_run[rt]);
                l_part[rt] += pv;
                const op_t h = (op_t)pv;
                ph[rt][i] = h; pl[rt][i] = (op_t)(pv - (float)h);
            }
        }
        // ---- U^T += E^T P^T over this wave's share of the columns on the 16x16x16 MFMA: A = one transposed 4-frame x 16-column block per column
        // block (lane (column n16, g): frames 4 sigma(g) .. + 3), B = this lane's four probabilities as they lie in the S^T accumulator (one
        // column block of E^T serves every row tile).  The reads of a group are waited for by hand, the wait carrying them as operands so that no
        // MFMA moves above it.
        constexpr int GR = (CB % 4 == 0) ? 4 : 2;
#pragma unroll
        for (int cb0 = 0; cb0 < CB; cb0 += GR) {
            xa_s16x4 r[GR];
#pragma unroll
            for (int j = 0; j < GR; j++) {
                const int c8 = 2 * (wv * CB + cb0 + j) + (p4 >> 1);   // 16-byte chunk that holds columns 16 (wv CB + cb) + 4 p4 .. + 3
                r[j] = xa_tr_read(sbase + xa_off<D>(4 * sg + q4, c8) + 8 * (p4 & 1));
            }
            if (GR == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]));
#pragma unroll
            for (int j = 0; j < GR; j++)
#pragma unroll
                for (int rt = 0; rt < RT; rt++) {
                    u[rt][cb0 + j] = XaMfmaK16<op_t>::run(r[j], ph[rt], u[rt][cb0 + j]);
                    u[rt][cb0 + j] = XaMfmaK16<op_t>::run(r[j], pl[rt], u[rt][cb0 + j]);
                }
        }
    }
    // the last leaf that holds frames, then the empty partials (U = 0, l = 0, m = -1e30: weight 0 in the merge) of the leaves a short clip does not reach
    for (; leaf < leaf0 + lpw; ) flush(leaf++);
}

template <int D, int NSLOT, bool PAIR, int WV = 4, int RT = 1>
__global__ __launch_bounds__(64 * WV, 8 / WV) void k_xattn_absorbed(XaArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char xa_smem[];   // NSLOT tiles | WV x RT x 1 KB of partial S^T
    xattn_absorbed_body<D, NSLOT, PAIR, WV, RT>(A, xa_smem);
}
// dynamic LDS of an instantiation; the waves and row tiles of a width
constexpr size_t xa_lds(int d, int nslot) { return (size_t)nslot * XA_TF * d * 2 + (d > 1024 ? 8 * 2 : 4) * 1024; }
constexpr int xa_waves(int d) { return d > 1024 ? 8 : 4; }

// The query projection and Q' in ONE launch: grid (heads, ceil(n / 16)), 4 waves.
//   step 1  q_h^T[i (64)][clip (16)] = Wq[h 64 + i][:] ln[clip][:] + bq, K = d: wave w takes every fourth k-step for all 64 rows i, the four partial sums
//           meet in LDS (added in wave order); rounded to op_t as the reference's fp16 Linear does and parked in LDS [clip][64]
//   step 2  Q'^T[j][clip] = Wk^T[j][h 64 + k] q_h[clip][k], K = 64: wave w owns d / 4 of the rows j; hi + lo out
// Every weight fragment a wave needs is requested before the first MFMA (one memory round trip for both steps): 12 us against 9 + 9 for
// the projection and a separate Q' launch.
// The cross-attention LayerNorm runs here too (k_layernorm's arithmetic, operation for operation: the same bits): every workgroup normalises its own 16
// rows of the residual stream into LDS -- twelve heads repeat the work of one 5 us launch, which is cheaper than the launch.
// PCE_NO_PK_F32: the pair sums of the LayerNorm ((x + y) + (z + w)) compile to v_pk_add_f32 ... op_sel:[0,1] op_sel_hi:[1,0], the form that goes wrong
// beside MFMA waves -- which other workgroups of this very launch are executing (see k_logmel_frames); no packed fp32 instructions in this kernel.
template <int D>
__global__ __launch_bounds__(256) PCE_NO_PK_F32 void k_xq_fused(const float *__restrict__ resid, const float *__restrict__ ln_w, const float *__restrict__ ln_b, const op_t *__restrict__ wq,
                                                   const float *__restrict__ bq, const op_t *__restrict__ wkT, int n, float scale, const int *__restrict__ skip,
                                                   op_t *__restrict__ qp_hi, op_t *__restrict__ qp_lo, int rows /* R of XaArgs */)
{
    constexpr int KW = D / 128, JB = D / 64;                        // step 1: k-steps per wave (every fourth one); step 2: 16-row blocks of j per wave
    __shared__ __attribute__((aligned(16))) op_t qs[16][64 + 8];
    __shared__ float red[4][4][64][4];                            // step 1's partial sums [wave][i block][lane][4]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n16 = lane & 15, g = lane >> 4;
    const int h = blockIdx.x, c = 16 * blockIdx.y + n16;
    __shared__ __attribute__((aligned(16))) op_t lns[16][D + 8];   // LayerNorm of the workgroup's 16 rows (row pitch 2 D + 16 bytes: the 16 rows of a fragment read hit different banks)
    const op_t *ar = wq + (int64_t)(h * 64 + n16) * D + 8 * g;
    opx8 kf[JB][2];                                               // step 2's weights: requested first, used last
#pragma unroll
    for (int jb = 0; jb < JB; jb++)
#pragma unroll
        for (int ks = 0; ks < 2; ks++) kf[jb][ks] = *reinterpret_cast<const opx8 *>(wkT + (int64_t)(wv * (D / 4) + 16 * jb + n16) * D + h * 64 + 32 * ks + 8 * g);
    {
        opx8 af[KW][4], bf[KW];
#pragma unroll
        for (int k = 0; k < KW; k++) {
            const int ks = 4 * k + wv;
#pragma unroll
            for (int ib = 0; ib < 4; ib++) af[k][ib] = *reinterpret_cast<const opx8 *>(ar + (int64_t)16 * ib * D + 32 * ks);
        }
        {   // LayerNorm of rows 4 wv .. 4 wv + 3 (one wave per row at a time, as k_layernorm: two-pass statistics in fp32)
            constexpr int NV = D / 4, NI = (NV + 63) / 64;
            float4 v[4][NI];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int rc = 16 * (int)blockIdx.y + 4 * wv + r;
                const float4 *xr = reinterpret_cast<const float4 *>(resid + (int64_t)(rc < n ? rc : n - 1) * D);
#pragma unroll
                for (int i = 0; i < NI; i++) { const int idx = lane + 64 * i; v[r][i] = idx < NV ? xr[idx] : make_float4(0.f, 0.f, 0.f, 0.f); }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float sm = 0.f;
#pragma unroll
                for (int i = 0; i < NI; i++) sm += (v[r][i].x + v[r][i].y) + (v[r][i].z + v[r][i].w);
                sm = wave_dpp_sum_f32(sm);
                const float mean = sm / (float)D;
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < NI; i++)
                    if (lane + 64 * i < NV) {
                        const float a0 = v[r][i].x - mean, a1 = v[r][i].y - mean, a2 = v[r][i].z - mean, a3 = v[r][i].w - mean;
                        q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                    }
                q = wave_dpp_sum_f32(q);
                const float inv = rsqrtf(q / (float)D + 1e-5f);
#pragma unroll
                for (int i = 0; i < NI; i++) {
                    const int idx = lane + 64 * i;
                    if (idx < NV) {
                        const float4 ww = reinterpret_cast<const float4 *>(ln_w)[idx], bb = reinterpret_cast<const float4 *>(ln_b)[idx];
                        xa_opx4 o;
                        o[0] = (op_t)((v[r][i].x - mean) * inv * ww.x + bb.x); o[1] = (op_t)((v[r][i].y - mean) * inv * ww.y + bb.y);
                        o[2] = (op_t)((v[r][i].z - mean) * inv * ww.z + bb.z); o[3] = (op_t)((v[r][i].w - mean) * inv * ww.w + bb.w);
                        *reinterpret_cast<xa_opx4 *>(&lns[4 * wv + r][4 * idx]) = o;
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KW; k++) bf[k] = *reinterpret_cast<const opx8 *>(&lns[n16][32 * (4 * k + wv) + 8 * g]);
#pragma unroll
        for (int ib = 0; ib < 4; ib++) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < KW; k++) a = mfma16(af[k][ib], bf[k], a);
            *reinterpret_cast<f32x4 *>(red[wv][ib][lane]) = a;
        }
    }
    __syncthreads();
    {
        f32x4 a = *reinterpret_cast<const f32x4 *>(red[0][wv][lane]);
#pragma unroll
        for (int w2 = 1; w2 < 4; w2++) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(red[w2][wv][lane]);
            a[0] += v[0]; a[1] += v[1]; a[2] += v[2]; a[3] += v[3];
        }
        xa_opx4 q4;
        const int i0 = 16 * wv + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; e++) q4[e] = (op_t)(a[e] + bq[h * 64 + i0 + e]);
        *reinterpret_cast<xa_opx4 *>(&qs[n16][i0]) = q4;
    }
    __syncthreads();
    opx8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ks++) qf[ks] = *reinterpret_cast<const opx8 *>(&qs[n16][32 * ks + 8 * g]);
    const bool dead = c >= n || (skip && skip[c]);
#pragma unroll
    for (int jb = 0; jb < JB; jb++) {
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        r = mfma16(kf[jb][0], qf[0], r);
        r = mfma16(kf[jb][1], qf[1], r);
        if (dead) continue;
        xa_opx4 h4, l4;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            // v is made opaque: left to itself the compiler converts the STORED hi from the fp32 product (v_mul_f32, v_cvt_pk_f16_f32) but takes the hi
            // it subtracts from the product fused into the conversion (v_fma_mixlo_f16: one rounding of the exact product).  Where the fp32 product
            // is a tie of the fp16 grid -- one element in 2^13 -- the two differ by a step of hi and hi + lo missed v by that step (fp16 build;
            // tests/test_gpu_xattn.py reads the query's bits back through Wk = I and found it)
            float v = r[e] * scale;
            asm volatile("" : "+v"(v));
            h4[e] = (op_t)v; l4[e] = (op_t)(v - (float)h4[e]);
        }
        const int64_t o = ((int64_t)c * rows + h) * D + wv * (D / 4) + 16 * jb + 4 * g;
        *reinterpret_cast<xa_opx4 *>(qp_hi + o) = h4;
        *reinterpret_cast<xa_opx4 *>(qp_lo + o) = l4;
    }
}

// out^T blocks: D[i (16)][clip (16)] = Wv[h 64 + i][j] U[clip][h][j], K = d, U merged from the splits' partials on the fly:
// U = sum_s 2^(m_s - m) u_s / sum_s 2^(m_s - m) l_s, as hi + lo pairs of op_t.  Grid (heads, ceil(n / 16)), 4 waves: wave w takes every fourth
// k-step of 32 for all four 16-row blocks of the head's 64 rows i -- every load of a wave is independent of the others, one memory round trip --
// and the four partial sums meet in LDS (added in wave order: the same bits every run).
template <int D, bool PAIRS>                                 // PAIRS: the partials are the two pair nodes (written by the PAIR kernels); else the four leaves
__global__ __launch_bounds__(256) void k_uv_absorb(const float *__restrict__ u_part, const float *__restrict__ ml_part, const op_t *__restrict__ wv_w,
                                                    const float *__restrict__ bv, int n, const int *__restrict__ skip, op_t *__restrict__ out, int64_t out_ld,
                                                    int rows /* R of XaArgs */)
{
    constexpr int KW = D / 128, NS = PAIRS ? XA_LEAVES / 2 : XA_LEAVES;   // k-steps per wave; nodes per clip in the buffer
    __shared__ float red[4][4][64][4];                            // [wave][i block][lane][4]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n16 = lane & 15, g = lane >> 4;
    const int h = blockIdx.x, c = 16 * blockIdx.y + n16, cc = c < n ? c : n - 1;
    const bool dead = c >= n || (skip && skip[c]);
    // the weights of the tree (L0 + L1) + (L2 + L3) for this (clip, head): w[s] scales node s inside its pair, wp[] the two pairs at the root
    float w[4] = {1.f, 1.f, 1.f, 1.f}, wp[2], inv;
    {
        float mv[NS], lv[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) { const float *mp = ml_part + (((int64_t)cc * NS + s) * rows + h) * 2; mv[s] = mp[0]; lv[s] = mp[1]; }
        float pm[2], pl[2];
        if (PAIRS) { pm[0] = mv[0]; pm[1] = mv[NS - 1]; pl[0] = lv[0]; pl[1] = lv[NS - 1]; }
        else {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                xa_merge_w(mv[2 * q], mv[(2 * q + 1) % NS], pm[q], w[2 * q], w[2 * q + 1]);
                pl[q] = xa_merge_v(lv[2 * q], w[2 * q], lv[(2 * q + 1) % NS], w[2 * q + 1]);
            }
        }
        float mr;
        xa_merge_w(pm[0], pm[1], mr, wp[0], wp[1]);
        inv = 1.0f / xa_merge_v(pl[0], wp[0], pl[1], wp[1]);
    }
    const float *up = u_part + ((int64_t)cc * NS * rows + h) * D + 8 * g;
    const op_t *wr = wv_w + (int64_t)(h * 64 + n16) * D + 8 * g;
    // every load of a wave is issued before the first use (one memory round trip: the partials and the weight fragments are independent of each other)
    f32x4 x[KW][NS][2];
    opx8 wf[KW][4];
#pragma unroll
    for (int k = 0; k < KW; k++) {
        const int ks = 4 * k + wv;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            x[k][s][0] = *reinterpret_cast<const f32x4 *>(up + (int64_t)s * rows * D + 32 * ks);
            x[k][s][1] = *reinterpret_cast<const f32x4 *>(up + (int64_t)s * rows * D + 32 * ks + 4);
        }
#pragma unroll
        for (int ib = 0; ib < 4; ib++) wf[k][ib] = *reinterpret_cast<const opx8 *>(wr + (int64_t)16 * ib * D + 32 * ks);
    }
    f32x4 a[4];
#pragma unroll
    for (int ib = 0; ib < 4; ib++) a[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KW; k++) {
        // U[e] of the root, element by element: the pair nodes (from the buffer, or merged here from two leaves), the root, 1 / l
        opx8 uh, ul;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            float p0, p1;
            if (PAIRS) { p0 = x[k][0][e >> 2][e & 3]; p1 = x[k][NS - 1][e >> 2][e & 3]; }
            else {
                p0 = xa_merge_v(x[k][0][e >> 2][e & 3], w[0], x[k][1 % NS][e >> 2][e & 3], w[1]);
                p1 = xa_merge_v(x[k][2 % NS][e >> 2][e & 3], w[2], x[k][3 % NS][e >> 2][e & 3], w[3]);
            }
            const float v = dead ? 0.f : xa_merge_v(p0, wp[0], p1, wp[1]) * inv;
            uh[e] = (op_t)v; ul[e] = (op_t)(v - (float)uh[e]);
        }
#pragma unroll
        for (int ib = 0; ib < 4; ib++) { a[ib] = mfma16(wf[k][ib], uh, a[ib]); a[ib] = mfma16(wf[k][ib], ul, a[ib]); }
    }
#pragma unroll
    for (int ib = 0; ib < 4; ib++) *reinterpret_cast<f32x4 *>(red[wv][ib][lane]) = a[ib];
    __syncthreads();
    f32x4 r = *reinterpret_cast<const f32x4 *>(red[0][wv][lane]);
#pragma unroll
    for (int w2 = 1; w2 < 4; w2++) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(red[w2][wv][lane]);
        r[0] += v[0]; r[1] += v[1]; r[2] += v[2]; r[3] += v[3];
    }
    if (dead) return;
    xa_opx4 o4;
    const int i0 = h * 64 + 16 * wv + 4 * g;
#pragma unroll
    for (int i = 0; i < 4; i++) o4[i] = (op_t)(r[i] + bv[i0 + i]);
    *reinterpret_cast<xa_opx4 *>(out + (int64_t)c * out_ld + i0) = o4;
}

// out[j][i] = in[i][j] (d x d, op_t): Wk^T at load time
__global__ void k_transpose_sq(const op_t *__restrict__ in, op_t *__restrict__ out, int d)
{
    __shared__ op_t t[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) t[r][tx] = in[(int64_t)(by + r) * d + bx + tx];
    __syncthreads();
    for (int r = ty; r < 32; r += 8) out[(int64_t)(bx + r) * d + by + tx] = t[tx][r];
}
