// pce_attention.inc -- the flash attention forward and its launchers (included by pce_whisper_impl.inc inside its anonymous namespace).
// ---------------------------------------------------------------------------
// attention forward, transposed formulation (attn_block16 below).
//   S^T = K Q^T   (keys on the accumulator rows, queries on its columns = lanes)
//   O^T = V^T P^T (P^T is consumed straight out of the S^T accumulator registers as the B operand: no LDS round trip, no
//                  cross-lane softmax reductions except the exchanges between lane groups)
// One workgroup = 4 waves x 32 queries of one (clip, head); K [64 keys][64 d] and V^T [64 d][64 keys]
// tiles stream through LDS by DMA (global_load_lds), double buffered, XOR-swizzled like the GEMM operands.
// ---------------------------------------------------------------------------
constexpr int AT_QB = 128;                  // queries per workgroup

struct AttnArgs {
    const op_t *q; int64_t q_ld;            // query row i of clip c: q + (q_row0[c] + i) * q_ld + head * 64
    const op_t *k; int64_t k_ld;            // key row j:             k + (k_row0[c] + j) * k_ld + head * 64
    const op_t *vt; int64_t vt_clip; int vt_sp;   // V^T: vt + c * vt_clip + (head * 64 + d) * vt_sp + j
    const int *q_row0, *q_len, *k_row0, *k_len;   // per clip
    op_t *out; int64_t out_ld;              // out + (q_row0[c] + i) * out_ld + head * 64
    int causal;                             // key j visible to query i only if j <= i
    int *fell_back;                         // (self-test only, else null) counts the workgroups of k_attention_lean16 that re-ran on the exact path
};

// ---------------------------------------------------------------------------
// The tile loop (round 4, first on v_mfma_f32_32x32x16 as k_attention_lean): less than half of k_attention's vector instructions per tile.  Per 64-key tile a wave issues
// 16 MFMAs and, in k_attention, about 200 VALU instructions; MFMAs and VALU instructions of all waves of a SIMD share one issue port
// (v_fma 4 cycles, v_exp 8, an MFMA 8 of its 32: MI355X_MICROARCH.md "vector-instruction ISSUE cost"), and with three waves per SIMD the
// PMC counters put k_attention's issue port at 96 % busy (SQ_ACTIVE_INST_ANY / SQ_WAVE_CYCLES = 0.32 per wave): it is instruction-count
// bound.  Removed from the tile loop:
//   * the running maximum.  exp2(s c - m) needs SOME reference m per query, not the maximum: softmax is invariant under the choice and
//     fp32 / op_t share an 8-bit exponent, so with m fixed at the query's maximum over TILE 0 nothing is lost until a later score exceeds
//     m by 127 / c.  That is detected (a non-finite row sum) and the workgroup then runs again on the exact path (EXACT = true: running
//     maximum, accumulator rescale, VALU row sums) -- never on Whisper's logits; tests drive it with synthetic ones and force it;
//   * the row sums: a 17th..20th MFMA per tile against a constant "row 0 = ones" fragment accumulates sum_j P[q][j] in the matrix pipe
//     (which has slack) instead of 32 v_add / 16 v_pk_add (which has none); the sums are over the op_t P the second product consumes;
//   * address arithmetic: K / V^T tiles arrive by LDS-DMA through buffer resources (constant per-lane offsets, one scalar offset per
//     tile; rows past the last key read as zeros and are masked like any invisible key), fragment addresses are loop invariants.
// Same workgroup shape, ring and register budget as k_attention (4 waves x 32 queries, 3 slots = 48 KB, three workgroups per CU).
// Measured, 256 clips x 12 heads x 1500^2: 2.56 -> 2.25 ms per launch.  Tried on the way and dropped: the next tile's S^T MFMAs
// interleaved with this tile's exponentials inside one wave (two score sets in registers, 4 slots, two workgroups per CU): 2.59 ms with or
// without the instruction diet -- waves then wait on LDS-DMA / barriers (SQ_WAIT_ANY 0.41) with too few partners to cover them; the same
// with eight waves per workgroup (half the DMA instructions per wave): 3.0 ms.
// ---------------------------------------------------------------------------
// attn_block16 (round 5): the same workgroup (4 waves x 32 queries, 64-key tiles, the same ring, the same staging instructions) on
// v_mfma_f32_16x16x32.  Why: (a) the row-sum products against the "row 0 = ones" fragment waste 15 of 16 rows instead of 31 of 32 -- 4
// MFMAs of 16 cycles per tile instead of 4 of 32, and the ablation of round 4 priced those four at 5.5 of the kernel's 30.8 ms per step;
// (b) MI355X_MICROARCH.md "DVFS give-back (7)": under the power limit these kernels run against, the 16x16x32 loop holds a higher clock.
// Per tile and wave: 16 MFMAs for S^T (4 key blocks x 2 query blocks x 2 k-steps of 32 dims), 16 for O^T += V^T P^T (4 d blocks x 2
// query blocks x 2 k-steps of 32 keys), 4 for the row sums: 576 MFMA cycles against 640.
// Layouts.  D = A B of 16x16x32: lane (n = lane & 15, g = lane >> 4) supplies A[m = n][8g .. 8g + 7] and B[8g .. 8g + 7][n], and holds
// D[4g + i][n] in register i.  S^T block (kb, qb) therefore leaves, in lane (query n, group g), the scores of the four keys on block rows
// 4g .. 4g + 3; the B operand of the second product wants, in the same lane, eight keys of one 32-key k-step.  Registers of blocks kb = 2s
// and 2s + 1 concatenated ARE such an operand if block row rho = 4g + i of block 2s + b stands for key 32s + 8g + 4b + i: the K rows are
// staged into LDS in that order (the LDS-DMA source row is free per lane: row R of the slot holds key kappa(R)), so the K fragments are
// read from natural, conflict-free rows and the V^T fragment of lane (d, g) is one contiguous 16-byte read of keys 32s + 8g .. + 7.
// No cross-lane movement, no LDS round trip for P.  Softmax does not care about the order of the keys inside a tile.
// ---------------------------------------------------------------------------
template <bool EXACT, bool NT>
__device__ __forceinline__ bool attn_block16(const AttnArgs &A, op_t *smem, int bx, int head, int clip)
{
    constexpr int NS = 3, DPW = 4;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, g = lane >> 4;
    const int Sq = A.q_len[clip], Sk = A.k_len[clip];
    const int q0 = bx * AT_QB + wv * 32;
    const op_t *qbase = A.q + (int64_t)A.q_row0[clip] * A.q_ld + head * 64;
    const op_t *kbase = A.k + (int64_t)A.k_row0[clip] * A.k_ld + head * 64;
    const op_t *vtbase = A.vt + (int64_t)clip * A.vt_clip + (int64_t)head * 64 * A.vt_sp;
    const int kld = (int)A.k_ld, vsp = A.vt_sp;
    const __amdgpu_buffer_rsrc_t rsK = __builtin_amdgcn_make_buffer_rsrc(const_cast<op_t *>(kbase), 0, ((Sk - 1) * kld + 64) * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(const_cast<op_t *>(vtbase), 0, 64 * vsp * 2, 0x00020000);
    int voffK[2], voffV[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int row = (wv + 4 * i) * 8 + (lane >> 3), c8 = swz_chunk(row, lane & 7) * 8;
        const int kb = row >> 4, rho = row & 15;
        const int key = 32 * (kb >> 1) + 8 * (rho >> 2) + 4 * (kb & 1) + (rho & 3);     // kappa(row): the key LDS row `row` of a K slot holds
        voffK[i] = (key * kld + c8) * 2; voffV[i] = (row * vsp + c8) * 2;
    }
    auto stage = [&](int t) {
        op_t *sK = smem + (t % NS) * (2 * 64 * 64), *sV = sK + 64 * 64;
        const int key0 = t * 64;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            // NT: a launch with ONE query block per (clip, head) -- the decoder's cross-attention -- reads every K / V^T byte exactly once: the
            // non-temporal policy (sc0 | nt) streams them past the caches (profiles/r05/xattn_absorb.txt: +14 % on such a stream)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsK, (__attribute__((address_space(3))) void *)(sK + (wv + 4 * i) * 8 * 64), 16, voffK[i], key0 * kld * 2, 0, NT ? 3 : 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsV, (__attribute__((address_space(3))) void *)(sV + (wv + 4 * i) * 8 * 64), 16, voffV[i], key0 * 2, 0, NT ? 3 : 0);
        }
    };
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    opx8 qf[2][2];                                              // [query block][k-step of 32 dims]
    int my_q[2];
#pragma unroll
    for (int qb = 0; qb < 2; qb++) {
        my_q[qb] = q0 + 16 * qb + n16;
        int qr = my_q[qb]; if (qr >= Sq) qr = Sq - 1;
        const op_t *qp = qbase + (int64_t)qr * A.q_ld;
#pragma unroll
        for (int ks = 0; ks < 2; ks++) qf[qb][ks] = *reinterpret_cast<const opx8 *>(qp + 32 * ks + 8 * g);
    }
    opx8 ones;                                                 // A fragment "row 0 = ones, rows 1..15 = 0" of the row-sum MFMA
#pragma unroll
    for (int j = 0; j < 8; j++) ones[j] = (op_t)(n16 == 0 ? 1.0f : 0.0f);
    f32x4 o[4][2], osum[2];
#pragma unroll
    for (int db = 0; db < 4; db++) { o[db][0] = z4; o[db][1] = z4; }
    osum[0] = z4; osum[1] = z4;
    float m_run[2] = {-1e30f, -1e30f}, l_run[2] = {0.f, 0.f};
    const float sl2 = 0.125f * 1.4426950408889634f;
    int k_need = Sk;
    if (A.causal) k_need = min(Sk, bx * AT_QB + AT_QB);
    const int nt = (k_need + 63) / 64;
    int kaddr[4][2], vaddr[4][2];                                // LDS addresses of this lane's fragments inside a slot (elements)
#pragma unroll
    for (int b4 = 0; b4 < 4; b4++)
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const int row = 16 * b4 + n16;
            kaddr[b4][ks] = row * 64 + swz_chunk(row, 4 * ks + g) * 8;
            vaddr[b4][ks] = 64 * 64 + row * 64 + swz_chunk(row, 4 * ks + g) * 8;
        }
    stage(0);
    if (nt > 1) stage(1);
    for (int kt = 0; kt < nt; kt++) {
        if (kt + 1 < nt) __builtin_amdgcn_s_waitcnt(0x0F70 | DPW); else __builtin_amdgcn_s_waitcnt(0x0F70 | 0);
        __builtin_amdgcn_s_barrier();
        if (kt + 2 < nt) stage(kt + 2);
        const op_t *sC = smem + (kt % NS) * (2 * 64 * 64);
        f32x4 sc[4][2];
#pragma unroll
        for (int kb = 0; kb < 4; kb++)
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                const opx8 kf = *reinterpret_cast<const opx8 *>(&sC[kaddr[kb][ks]]);
#pragma unroll
                for (int qb = 0; qb < 2; qb++) sc[kb][qb] = mfma16(kf, qf[qb][ks], ks == 0 ? z4 : sc[kb][qb]);
            }
        if ((kt * 64 + 63 >= Sk) || (A.causal && kt * 64 + 63 > q0)) {                          // wave-uniform: an edge tile
#pragma unroll
            for (int kb = 0; kb < 4; kb++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int key = kt * 64 + 32 * (kb >> 1) + 8 * g + 4 * (kb & 1) + i;
#pragma unroll
                    for (int qb = 0; qb < 2; qb++) {
                        const bool vis = key < Sk && (!A.causal || key <= my_q[qb]);
                        sc[kb][qb][i] = vis ? sc[kb][qb][i] : -1e30f;
                    }
                }
        }
        if (EXACT || kt == 0) {
            float mx[2];
#pragma unroll
            for (int qb = 0; qb < 2; qb++) {
                float m = sc[0][qb][0];
#pragma unroll
                for (int kb = 0; kb < 4; kb++)
#pragma unroll
                    for (int i = 0; i < 4; i++) m = fmaxf(m, sc[kb][qb][i]);
                m = m > -1e29f ? m * sl2 : -1e30f;
                m = fmaxf(m, __shfl_xor(m, 16, 64));
                m = fmaxf(m, __shfl_xor(m, 32, 64));
                mx[qb] = fmaxf(m_run[qb], m);
            }
            if (__builtin_amdgcn_ballot_w64(mx[0] > m_run[0] || mx[1] > m_run[1]) != 0) {
#pragma unroll
                for (int qb = 0; qb < 2; qb++) {
                    const float corr = __builtin_amdgcn_exp2f(m_run[qb] - mx[qb]);   // (tile 0: everything it scales is still zero)
                    l_run[qb] *= corr;
#pragma unroll
                    for (int db = 0; db < 4; db++)
#pragma unroll
                        for (int i = 0; i < 4; i++) o[db][qb][i] *= corr;
                    m_run[qb] = mx[qb];
                }
            }
            // fp16 operands: P = 2^(s c - m) must stay below 65 504 = 2^16 (bf16 has fp32's exponent range).  The fixed reference sits
            // 4 octaves ABOVE the first tile's maximum: a later score may exceed that maximum by 2^20 (13.9 nats) before the row overflows
            // (and the workgroup re-runs exactly), at the price of flushing weights below 2^-20 of the reference to zero
            // (<= 1 500 keys x 1e-6: 0.15 % of a row in the worst case; the exact path, like the reference, cuts at 2^-24).
            if (!EXACT && std::is_same<op_t, _Float16>::value) { m_run[0] += 4.0f; m_run[1] += 4.0f; }
        }
        float rs[2] = {0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; kb++)
#pragma unroll
            for (int qb = 0; qb < 2; qb++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(sc[kb][qb][i], sl2, -m_run[qb]));
                    sc[kb][qb][i] = pv;
                    if (EXACT) rs[qb] += pv;
                }
        if (EXACT) {
#pragma unroll
            for (int qb = 0; qb < 2; qb++) {
                float sum = rs[qb];
                sum += __shfl_xor(sum, 16, 64);
                sum += __shfl_xor(sum, 32, 64);
                l_run[qb] += sum;
            }
        }
        // O^T += V^T P^T (and the row sums): k-step s covers keys 32 s .. 32 s + 31; B = the registers of S^T blocks 2 s and 2 s + 1
        opx8 vf[4][2];
#pragma unroll
        for (int db = 0; db < 4; db++)
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) vf[db][s2] = *reinterpret_cast<const opx8 *>(&sC[vaddr[db][s2]]);
#pragma unroll
        for (int s2 = 0; s2 < 2; s2++)
#pragma unroll
            for (int qb = 0; qb < 2; qb++) {
                opx8 pf;
#pragma unroll
                for (int i = 0; i < 4; i++) { pf[i] = (op_t)sc[2 * s2][qb][i]; pf[4 + i] = (op_t)sc[2 * s2 + 1][qb][i]; }
#pragma unroll
                for (int db = 0; db < 4; db++) o[db][qb] = mfma16(vf[db][s2], pf, o[db][qb]);
                if (!EXACT) osum[qb] = mfma16(ones, pf, osum[qb]);
            }
    }
    if (!EXACT) {                                               // row 0 of the row-sum product: register 0 of lanes 0..15
        l_run[0] = __shfl(osum[0][0], n16, 64);
        l_run[1] = __shfl(osum[1][0], n16, 64);
    }
    const bool ok = EXACT || (((l_run[0] > 0.f && l_run[0] < 1.0e30f) || my_q[0] >= Sq) && ((l_run[1] > 0.f && l_run[1] < 1.0e30f) || my_q[1] >= Sq));
    if (!EXACT && __syncthreads_or(!ok)) return false;           // some row overflowed its fixed reference: the workgroup runs again, exactly
    // O^T block (db, qb): this lane holds d = 16 db + 4 g .. + 3 of query q0 + 16 qb + n16
    typedef __attribute__((ext_vector_type(4))) op_t opx4;
#pragma unroll
    for (int qb = 0; qb < 2; qb++) {
        if (my_q[qb] >= Sq) continue;
        const float inv = 1.0f / l_run[qb];
        op_t *op = A.out + ((int64_t)A.q_row0[clip] + my_q[qb]) * A.out_ld + head * 64;
#pragma unroll
        for (int db = 0; db < 4; db++) {
            opx4 v4;
#pragma unroll
            for (int i = 0; i < 4; i++) v4[i] = (op_t)(o[db][qb][i] * inv);
            *reinterpret_cast<opx4 *>(op + 16 * db + 4 * g) = v4;
        }
    }
    return true;
}

// Workgroups go to the 8 XCDs round robin by linear id, and the query blocks of one (clip, head) share its K / V^T through L2: every XCD gets a
// CONTIGUOUS range of (clip, head, query block) triples, so that the blocks that share keys meet in one L2 instead of eight.
// NT: a launch with one query block per (clip, head) (see attn_block16's staging).
template <bool NT>
__global__ __launch_bounds__(256, 3) void k_attention_lean16(AttnArgs A, int force_exact /* self-test only */)
{
    __shared__ __attribute__((aligned(1024))) op_t smem[3 * 2 * 64 * 64];
    const unsigned nx = gridDim.x, ny = gridDim.y, total = nx * ny * gridDim.z;
    const unsigned lin = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z), xcd = lin & 7u, per = total >> 3, rem = total & 7u;
    const unsigned logical = xcd * per + (xcd < rem ? xcd : rem) + (lin >> 3);
    const int bx = (int)(logical % nx), head = (int)((logical / nx) % ny), clip = (int)(logical / (nx * ny));
    if (bx * AT_QB >= A.q_len[clip]) return;
    if (!force_exact && attn_block16<false, NT>(A, smem, bx, head, clip)) return;
    if (!force_exact && A.fell_back && threadIdx.x == 0) atomicAdd(A.fell_back, 1);
    __syncthreads();
    attn_block16<true, NT>(A, smem, bx, head, clip);
}

static void launch_attention(pce_ctx *c, dim3 grid, const AttnArgs &a, double flops = 0.0, int force_exact = 0 /* self-test only */)
{
    // flops > 0: a launch the profiler brackets on its own (the encoder's); the decoder's small launches stay inside their composite entry
    KernelTimer kt(c, PCE_K_ATTENTION_LEAN, nullptr, flops);
    if (grid.x == 1) hipLaunchKernelGGL(k_attention_lean16<true>, grid, dim3(256), 0, c->stream, a, force_exact);
    else hipLaunchKernelGGL(k_attention_lean16<false>, grid, dim3(256), 0, c->stream, a, force_exact);
}
// The product's attention launch (the one place it fills an AttnArgs): H heads of n clips, up to q_rows queries each, out rows of H * 64
static void launch_attention_rows(pce_ctx *c, int n, int H, int q_rows, const op_t *q, int64_t q_ld, const op_t *k, int64_t k_ld, const op_t *vt, int vt_sp,
                                  const int *q_row0, const int *q_len, const int *k_row0, const int *k_len, op_t *out, int causal, double flops = 0.0)
{
    AttnArgs a{};
    a.q = q; a.q_ld = q_ld; a.k = k; a.k_ld = k_ld; a.vt = vt; a.vt_clip = (int64_t)H * 64 * vt_sp; a.vt_sp = vt_sp;
    a.q_row0 = q_row0; a.q_len = q_len; a.k_row0 = k_row0; a.k_len = k_len; a.out = out; a.out_ld = H * 64; a.causal = causal;
    launch_attention(c, dim3((unsigned)div_up(q_rows, AT_QB), (unsigned)H, (unsigned)n), a, flops);
}
