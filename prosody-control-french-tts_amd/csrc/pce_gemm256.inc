// pce_gemm256.inc -- persistent 256 x 256 tile GEMM for the big encoder projections (included by pce_whisper_impl.inc).
//
//   C[M][N] (op_t) = epilogue(A[M][K] * B[N][K]^T + bias),  A dense row-major (pitch K), N % 256 == 0, K % 64 == 0.
//
// Why another GEMM: the 128 x 256 kernel pulls (128 + 256) * 2 bytes of operands per 2 * 128 * 256 flops; the path that
// delivers freshly streamed lines into a CU's LDS sustains about 28 B/clk (tools/lab/dma_pat.hip), which caps it near
// 58 % of the MFMA rate; a 256 x 256 tile needs two thirds of those bytes.  What made 256 x 256 lose before (one workgroup
// per CU: nothing hides the pipeline fill and the epilogue of a 12-step K loop) is removed by making the kernel persistent:
//
//   * one workgroup per CU walks its output tiles as ONE flat sequence of 64-deep K-steps; the operand stream of the next
//     tile is already in flight while the current tile's accumulators are written, and never drains;
//   * a K-step is four 16 KB half-tiles (A rows 0-127 | A rows 128-255 | B rows 0-127 | B rows 128-255) in a ring of
//     2 x 4 slots (128 KB LDS); half-tiles arrive by LDS-DMA through buffer resources: the per-lane offset is a constant,
//     everything that moves is a scalar offset (no address arithmetic, no 64-bit pointers in VGPRs);
//   * 8 waves as 2 (M) x 4 (N); a wave owns 64 rows of EACH A half and 32 columns of EACH B half, so each of its four
//     64 x 32 quadrants touches one A half and one B half;
//   * round 3 (the ping-pong K-step): a K-step is four phases of [LDS reads of the phase's new fragments + one half-tile
//     staged + wait] barrier [16 MFMAs] barrier, and wave row 1 runs one barrier behind wave row 0, so the two waves of a SIMD are
//     always in opposite sections (kstep below); the rows meet for the epilogue.  1 006 -> 1 076 TFLOP/s over the encoder's
//     launches on one box (same-box A/B of the two builds), results bit-identical;
//   * rounds 2-3a ran two barriers per K-step with all eight waves in step: measured and retired, see profiles/r03;
//   * 64 fragment VGPRs + 128 accumulator VGPRs, no spills (205-217 VGPRs);
//   * MFMA operands are swapped (D^T = B A^T) and the B rows of every 32-row group are permuted at staging time, so a
//     lane ends up with 8 CONSECUTIVE COLUMNS of one row: rows leave as 16-byte buffer stores straight from the
//     accumulators.  The transposed-V variant does the mirror image (A rows permuted, operands in natural order): a
//     lane holds 8 consecutive ROWS (key positions) of one column;
//   * FEPI_RESID: the row-major epilogue also ADDS the tile to a 16-bit residual matrix, in place (C = R): the encoder's attention projection and fc2
//     update the fp16 residual stream themselves, x = r16(x + r16(acc + bias)), so no branch output is stored and the LayerNorm passes read the
//     stream once (k_add_layernorm without deltas); the tile's 16 residual pieces are loaded into the fragment registers, dead between two tiles;
//   * the bias vector lives in LDS behind the ring; the accumulators are cleared after the epilogue (starting a tile from the zero
//     constant is NOT safe: see the note in the K loop); workgroups start staggered over a tile time so that their store bursts do not coincide.
//
// Measured in the lab (tools/lab/gemm_flat.hip, uniform random operands, M = 384 000): 1.09-1.13 PFLOP/s at K = 768
// (QKV, fc1, out-proj shapes), 1.23 PFLOP/s at K = 3072, against 0.93-1.0 for the 128 x 256 kernel.
// What bounds it: a CU takes operands in at about 25 B/clk however they are issued (one 1 KB LDS-DMA instruction per ~40 cycles through the
// CU's one vector-memory address path: the kernel without MFMAs, fragment reads and stores runs 2 550 cycles per K-step), so a 256 x 256
// K-step (64 KB) cannot go under 2 560 cycles against 2 048 of MFMA issue: 80 % of the MFMA peak is this tile shape's ceiling, and a wave
// that is issuing its eight DMA instructions of a K-step issues no MFMAs meanwhile (only its partner on the SIMD does): measured K-steps
// take 3 900.  Loader waves would take the DMA issue out of the MFMA waves' streams, but need the VGPRs of a third wave per SIMD, which
// 128 accumulator registers per wave do not leave; smaller tiles with loader waves move 1.5 x the bytes per flop (ceiling 53 %).
// Where a K = 768 tile's 55 000 cycles go (in-kernel stamps, same harness): ten middle K-steps of 3 900 (2 048 of them MFMA issue; the
// operand stream alone runs at 2 550 per K-step), 4 000 issuing the epilogue's 16 stores, a 5 000-cycle stall at the end of the next
// K-step (the in-order vmcnt wait sees the stores first).  Tried against that and measured, none kept: the A operand three K-steps deep
// (10 slots, 160 KB): +2 / -1 / +4 % on the out-proj / fc1 / fc2 shapes; the epilogue split over the neighbouring K-steps (upper half of
// the tile between the MFMA groups of the last K-step's second half, lower half between those of the next tile's first half): 4 % slower;
// full-line (8 rows x 128 B) or non-temporal stores: +-1 %; operands addressed as if stored half-tile by half-tile (every DMA instruction 1 KB of
// consecutive bytes: the operand stream alone 10-17 % faster, the kernel 0-5 %: not worth re-laying out every activation); no per-group priority, or a static higher priority for the second wave row: +-1 %; the two wave rows (the partners on a SIMD) issuing their LDS-DMA at different points of a half (round 3): +-0.3 %.  A stamped
// middle K-step shows the two partner waves of a SIMD unbalanced (the older one waits about 600 cycles at each of the two barriers for the
// younger, whose MFMA groups take twice as long) and 700 cycles per K-step behind the in-order wait for the A half issued at the step's top.

constexpr int F_T = 256, F_K = 64, F_THREADS = 512;
constexpr int F_N_MAX = 6144;            // widest output launch_gemm_flat takes: the bias row of a tile column lives in LDS (ring + N floats)
constexpr int F_HALF = 128 * F_K;                          // elements of a half-tile (16 KB)
constexpr int F_RING_BYTES = 8 * F_HALF * 2;
enum { FEPI_BF16 = 0, FEPI_GELU = 1, FEPI_VT = 2, FEPI_SPLIT = 3, FEPI_RESID = 4 };
// FEPI_SPLIT (round 3): ONE launch for a projection whose leading columns leave row-major and whose trailing columns leave as the
// transposed-V image (encoder Q | K | V: N = 3 d, cross-attention K | V: N = 2 d).  The A panel is swept once instead of twice and the
// tile list of the two products is one stream (no second launch tail).  A tile of the transposed part is computed as the TRANSPOSED
// PROBLEM, V^T = W_v X^T: the weight rows take the A slots of the ring and the activation rows the B slots (a scalar select of the
// buffer resource and the base row per DMA; the per-lane offsets are the same), the K-step is the same code, and the row-major
// epilogue then writes rows n and 8 consecutive key positions per lane: the V^T image as it stands (bias per row, clip boundary
// as in the FEPI_VT form).  (Two K-step bodies -- one per MFMA operand order -- behind a scalar branch spilled 373 VGPRs.)

__device__ __forceinline__ int f_swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
__device__ __forceinline__ int f_perm32(int p) { return ((p >> 2) & 3) * 8 + (p >> 4) * 4 + (p & 3); }   // LDS row of a 32-row group -> matrix row

struct FCursor { int kofs, m0, n0, vt; };                  // vt: the tile's columns belong to the transposed part (FEPI_SPLIT; else constant)
// tile order: XCD x owns a contiguous chunk of the supertile-ordered list (sm x sn tiles per supertile); the workgroups
// of the XCD take consecutive entries, so that at any time they share a few A and B panels in that XCD's L2
struct FSched {
    int tiles_n, sm, sn, per_xcd, xcd, slot, wper, my_tiles;
    __device__ void init(int M, int N, int sm_, int sn_)
    {
        tiles_n = N / F_T; sm = sm_; sn = sn_;
        const int tiles_m = (M + F_T - 1) / F_T, tiles_m_pad = ((tiles_m + sm - 1) / sm) * sm;
        const int total = tiles_m_pad * tiles_n;
        per_xcd = (total + 7) >> 3; xcd = blockIdx.x & 7; slot = blockIdx.x >> 3; wper = gridDim.x >> 3;
        my_tiles = per_xcd > slot ? (per_xcd - slot + wper - 1) / wper : 0;
    }
    __device__ void tile(int it, int &m0, int &n0) const
    {
        const int lin = xcd * per_xcd + slot + it * wper;
        const int per = sm * sn, sup = lin / per, r = lin - sup * per;
        const int n_sn = tiles_n / sn;
        m0 = ((sup / n_sn) * sm + r / sn) * F_T; n0 = ((sup % n_sn) * sn + r % sn) * F_T;
    }
};

struct FFrags { opx8 RA[2][4], RB0[2][2], RB1[2][2]; };   // A sub-tile in use [k half][row block]; B of column half 0 / 1 [k half][col block]
struct FArgs {
    const op_t *A, *B; const float *bias; op_t *C;
    int M, N, K, ldc;                     // ldc: row pitch of C in elements (FEPI_BF16 / FEPI_GELU)
    int S, vt_sp;                         // FEPI_VT: rows per clip, padded key axis of the V^T image: C[(clip * N + n) * vt_sp + t]
    int sm, sn, stagger;
    op_t *C2; int vt_n0;                  // FEPI_SPLIT: columns >= vt_n0 (a multiple of 256) go to the V^T image C2[(clip * (N - vt_n0) + n - vt_n0) * vt_sp + t]
    const op_t *R;                        // FEPI_RESID: the residual rows, pitch ldc like C; may BE C (the encoder's stream, updated in place)
};

template <int N> __device__ __forceinline__ void f_wait_vm() { __builtin_amdgcn_s_waitcnt(((N >> 4) << 14) | 0x0F70 | (N & 15)); }
template <int N> __device__ __forceinline__ void f_wait_lgkm() { __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8)); }

template <int KK, int HALF>
__device__ __forceinline__ void f_read_A(FFrags &F, const op_t *dsm, const int (&ra)[2], int par)
{
    const op_t *s = dsm + ((HALF ? 1 : 0) * 2 + par) * F_HALF;
#pragma unroll
    for (int i = 0; i < 4; i++) F.RA[KK][i] = *reinterpret_cast<const opx8 *>(s + ra[KK] + i * 16 * F_K);
}
template <int KK, int HALF>
__device__ __forceinline__ void f_read_B(FFrags &F, const op_t *dsm, const int (&rb)[2], int par)
{
    const op_t *s = dsm + ((HALF ? 1 : 0) * 2 + par) * F_HALF;            // rb already points into the B region of the ring
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const opx8 v = *reinterpret_cast<const opx8 *>(s + rb[KK] + j * 16 * F_K);
        if (HALF) F.RB1[KK][j] = v; else F.RB0[KK][j] = v;
    }
}
template <bool VT, int HA, int HB, int KK>
__device__ __forceinline__ void f_mma8(f32x4 (&acc)[2][2][4][2], const FFrags &F)
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const opx8 b = HB ? F.RB1[KK][j] : F.RB0[KK][j];
            acc[HA][HB][i][j] = VT ? mfma16(F.RA[KK][i], b, acc[HA][HB][i][j])
                                   : mfma16(b, F.RA[KK][i], acc[HA][HB][i][j]);
        }
}

template <int EPI>
__global__ __launch_bounds__(F_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_gemm_flat(FArgs P)
{
    constexpr bool SPLIT = EPI == FEPI_SPLIT;
    extern __shared__ __attribute__((aligned(1024))) op_t dsm[];
    float *sbias = reinterpret_cast<float *>(dsm + 8 * F_HALF);
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wv >> 2, wc = wv & 3;
    const int fr = lane & 15, fq = lane >> 4;
    const int M = P.M, N = P.N, K = P.K;
    FSched S; S.init(M, N, P.sm, P.sn);
    const int nk = K / F_K;
    if (S.my_tiles == 0) return;
    for (int i = tid; i < N; i += F_THREADS) sbias[i] = P.bias ? P.bias[i] : 0.f;
    if (P.stagger > 0) {                                     // spread the workgroups' store bursts over a tile time
        const unsigned long long t0 = __builtin_amdgcn_s_memtime(), d = (unsigned long long)P.stagger * (unsigned)(S.slot * 8 + S.xcd) / 256u;
        while (__builtin_amdgcn_s_memtime() - t0 < d) __builtin_amdgcn_s_sleep(8);
    }
    // staging: a half-tile is 128 LDS rows x 128 B = 16 wave-instructions of 8 rows, 2 per wave (LDS rows r and r + 64)
    int voff_plain, voff_perm;                                // per-lane byte offset of a staged row: as it stands / with the 32-row-group permutation
    {
        const int row = wv * 8 + (lane >> 3), c8 = f_swz(row, lane & 7) * 8;        // (row + 64 has the same swizzle)
        const int prow = (row & ~31) + f_perm32(row & 31);
        voff_plain = (row * K + c8) * 2; voff_perm = (prow * K + c8) * 2;           // row-major tiles permute B, transposed tiles permute A
    }
    int ra[2], rb[2];
    {
        const int r_a = wr * 64 + fr, r_b = wc * 32 + fr;                            // + 16 i keeps the swizzle term
        ra[0] = r_a * F_K + f_swz(r_a, fq) * 8; ra[1] = r_a * F_K + f_swz(r_a, 4 + fq) * 8;
        rb[0] = r_b * F_K + f_swz(r_b, fq) * 8 + 4 * F_HALF; rb[1] = r_b * F_K + f_swz(r_b, 4 + fq) * 8 + 4 * F_HALF;
    }
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<op_t *>(P.A), 0, (int)((unsigned)M * (unsigned)K * 2u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<op_t *>(P.B), 0, (int)((unsigned)N * (unsigned)K * 2u), 0x00020000);
    const int ld2_64 = 64 * K * 2;
    FCursor pc1, pc2;                                       // K-steps s + 1 and s + 2
    int it1, kt1, it2, kt2;
    const int last_tile = S.my_tiles - 1;
    auto set_tile = [&](FCursor &c, int it) {
        S.tile(it < last_tile ? it : last_tile, c.m0, c.n0);
        c.vt = SPLIT ? (c.n0 >= P.vt_n0) : (EPI == FEPI_VT);
    };
    auto advance = [&](FCursor &c, int &it, int &kt) {      // past the end of the stream the last tile's addresses are re-issued into slots nobody reads
        if (++kt == nk) { kt = 0; ++it; set_tile(c, it); }
        c.kofs = kt * F_K;
    };
    auto issue = [&](const FCursor &c, int kind, int par) { // kind 0: A rows 0-127, 3: A rows 128-255, 1: B rows 0-127, 2: B rows 128-255
        op_t *slot = dsm + ((kind == 0 ? 0 : kind == 3 ? 1 : kind == 1 ? 2 : 3) * 2 + par) * F_HALF;
        const bool is_a = kind == 0 || kind == 3;
        const bool act = SPLIT ? (is_a != (c.vt != 0)) : is_a;           // this half-tile holds rows of the activation matrix (else of the weights)
        const unsigned soff = (unsigned)((act ? c.m0 : c.n0) + ((kind == 3 || kind == 2) ? 128 : 0)) * (unsigned)K * 2u + (unsigned)c.kofs * 2u;
        const int voff = ((EPI == FEPI_VT) == is_a) ? voff_perm : voff_plain;
#pragma unroll
        for (int i = 0; i < 2; i++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(act ? rsA : rsB, (__attribute__((address_space(3))) void *)(slot + (wv + 8 * i) * 8 * F_K), 16,
                                                     voff, (int)(soff + (unsigned)(i * ld2_64)), 0, 0);
    };
    f32x4 acc[2][2][4][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    FFrags F;

    // ---- epilogue (16 stores per lane)
    // Store-data hazard, seen on gfx950 with ROCm 7.2: hipcc lets the conversions of the NEXT row block overwrite the VGPRs of a
    // buffer_store_dwordx4 in the very next instruction; with the vector-memory queue busy (LDS-DMA in flight) the store had not read
    // all of its data yet: the first dword of the last lanes of every 16-lane group left as the bits of the next block's fp32 sum.
    // It came and went with the instruction schedule (tools/gemm_check.py found it; the laboratory build never showed it).  Wait states
    // after every store keep the data registers intact; sixteen stores x 16 cycles per tile cost nothing measurable.
#ifndef F_STORE_AUX
#define F_STORE_AUX 0          // cache policy of the tile stores (gfx950 aux bits: 1 sc0, 2 nt, 16 sc1)
#endif
#define F_STORE_GUARD { asm volatile("s_nop 7\n\ts_nop 7" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    constexpr bool HAS_RM = EPI != FEPI_VT, HAS_VT = EPI == FEPI_VT || SPLIT;
    const int Nv = SPLIT ? N - P.vt_n0 : N;                                          // columns of the V^T image
    op_t *const vt_ptr = SPLIT ? P.C2 : P.C;
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(P.C, 0, HAS_RM ? (int)((unsigned)M * (unsigned)P.ldc * 2u) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc(vt_ptr, 0, HAS_VT ? (int)((unsigned)(M / P.S) * (unsigned)Nv * (unsigned)P.vt_sp * 2u) : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(const_cast<op_t *>(EPI == FEPI_RESID ? P.R : P.C), 0,
                                                                         EPI == FEPI_RESID ? (int)((unsigned)M * (unsigned)P.ldc * 2u) : 0, 0x00020000);
    const int voffC = (fr * P.ldc + fq * 8) * 2, voffV = (fr * P.vt_sp + fq * 8) * 2;
    // row-major tile.  lane: row fr of the row block, 8 consecutive columns fq * 8 .. + 7 of the wave's 32-column group
    // FEPI_RESID: C[m][n] = (op_t)((float)R[m][n] + (float)(op_t)(acc + bias)): the rounded branch output added to the residual row and rounded
    // again, which is what k_add_layernorm computes from a stored branch output (x1 = r16(x + delta)), bit for bit.  The tile's 16 residual
    // pieces are loaded first, every lane the 16 bytes it will store (same resource size, same offsets: rows past M read zeros and their
    // stores are dropped), non-temporal: the stream is read once.  They take 64 VGPRs, and 64 are free here: in the ping-pong K-step every
    // fragment is re-read from LDS in phases 1-3, so FFrags is dead between a tile's last K-step and the next tile's first.
    // R may be C: a 16-byte piece is read and written by the same lane, the store takes its data from the load, and no other workgroup
    // touches the tile.
    // The counted waits that follow an epilogue (after_stores 1 and 2, and the plain count of a one-step K loop) stay as they are.  They
    // rely on ONE property of the in-order vmcnt queue: behind the last LDS-DMA instruction issued before the epilogue sit AT LEAST EPI_OPS
    // operations of the epilogue.  Loads only add to that number, so no wait can return early.  And no wait returns later either: piece i is
    // consumed by store i, so hipcc retires load i (and with it, in order, everything older: the other row's half-tiles of K-steps s + 1
    // and s + 2, issued up to four phases ago) before store i; when the epilogue ends, the queue holds its stores and nothing older, the
    // parent's state exactly.  after_stores == 1 then leaves this K-step's 8 DMA instructions + 16 stores in flight, after_stores == 2 waits
    // for A-bottom(s + 1) and so for every store; with nk == 1 the plain vmcnt(6) of the next tile's only K-step retires the stores.
    // (Issuing the first four loads a phase earlier, in phase 4 of the tile's last K-step where the B-right fragments are dead, with that step's
    // wait raised to vmcnt(10), measured 0.3 ms of GEMM per step less in the kernel statistics and nothing in the step time: profiles/r15.)
    auto store_rm = [&](int m0, int n0) {
        u32x4 rv[2][2][4];
        if constexpr (EPI == FEPI_RESID) {
#pragma unroll
            for (int hB = 0; hB < 2; hB++)
#pragma unroll
                for (int hA = 0; hA < 2; hA++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const unsigned soff = ((unsigned)(m0 + hA * 128 + wr * 64 + i * 16) * (unsigned)P.ldc + (unsigned)(n0 + hB * 128 + wc * 32)) * 2u;
                        rv[hB][hA][i] = __builtin_amdgcn_raw_buffer_load_b128(rsR, voffC, (int)soff, 2 /* nt */);
                    }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int hB = 0; hB < 2; hB++) {
            const float *bp = sbias + n0 + hB * 128 + wc * 32 + fq * 8;
            const float4 b0 = *reinterpret_cast<const float4 *>(bp), b1 = *reinterpret_cast<const float4 *>(bp + 4);
            const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int hA = 0; hA < 2; hA++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    opx8 o;
                    float t[8];
#pragma unroll
                    for (int e = 0; e < 8; e++) t[e] = acc[hA][hB][i][e >> 2][e & 3] + bv[e];
                    if (EPI == FEPI_GELU) gelu_exact8(t);
#pragma unroll
                    for (int e = 0; e < 8; e++) o[e] = (op_t)t[e];
                    if constexpr (EPI == FEPI_RESID) {
                        const opx8 r = __builtin_bit_cast(opx8, rv[hB][hA][i]);
#pragma unroll
                        for (int e = 0; e < 8; e++) o[e] = (op_t)((float)r[e] + (float)o[e]);
                    }
                    const unsigned soff = ((unsigned)(m0 + hA * 128 + wr * 64 + i * 16) * (unsigned)P.ldc + (unsigned)(n0 + hB * 128 + wc * 32)) * 2u;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rsC, voffC, (int)soff, F_STORE_AUX);
                    __builtin_amdgcn_sched_barrier(0);
                    F_STORE_GUARD
                }
        }
    };
    // transposed tile (n0 counts from the first transposed column; the bias vector is indexed with nb0 = its column in the launch).
    // lane: column fr of the column block, 8 consecutive rows (key positions) fq * 8 .. + 7 of a 32-row group: two 8-byte
    // stores (a group of 4 positions never straddles a clip: S % 4 == 0).  V^T element (clip, n, t) sits at ((clip Nv + n) vt_sp + t);
    // a tile spans at most one clip boundary (S >= 256): positions past it move on by one clip, i.e. by (Nv vt_sp - S) elements.
    // Rows past M belong to a clip past the last one: outside the resource, dropped.
    auto store_vt = [&](int m0, int n0, int nb0) {
        typedef __attribute__((ext_vector_type(4))) op_t opx4;
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        const int clip0 = m0 / P.S, t_tile = m0 - clip0 * P.S;
        const int wrap = (Nv * P.vt_sp - P.S) * 2;
#pragma unroll
        for (int hB = 0; hB < 2; hB++)
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int n_s = n0 + hB * 128 + wc * 32 + j * 16;
                const float bv = sbias[nb0 + hB * 128 + wc * 32 + j * 16 + fr];
                const unsigned col = ((unsigned)clip0 * (unsigned)Nv + (unsigned)n_s) * (unsigned)P.vt_sp;
#pragma unroll
                for (int hA = 0; hA < 2; hA++)
#pragma unroll
                    for (int g = 0; g < 2; g++) {
                        // the lane's 8 positions t_g + fq * 8 .. + 7 (row blocks 2 g and 2 g + 1) are contiguous in V^T: ONE 16-byte store, unless the
                        // clip boundary cuts this 32-position group in the middle of a lane's 8 (then two 8-byte stores, as groups of 4 never straddle)
                        const int t_g = t_tile + hA * 128 + wr * 64 + g * 32, rel = P.S - t_g;              // wave-uniform
                        if (!(rel > 0 && rel < 32 && (rel & 7) == 4)) {
                            opx8 o;
#pragma unroll
                            for (int r = 0; r < 8; r++) o[r] = (op_t)(acc[hA][hB][2 * g + (r >> 2)][j][r & 3] + bv);
                            const int voff = voffV + ((t_g + fq * 8 >= P.S) ? wrap : 0);
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rsV, voff, (int)((col + (unsigned)t_g) * 2u), F_STORE_AUX);
                            F_STORE_GUARD
                        } else {
#pragma unroll
                            for (int h = 0; h < 2; h++) {             // accumulator of LDS row block i = 2 g + h: rows g * 32 + fq * 8 + h * 4 + r
                                const int t_s = t_g + h * 4;
                                opx4 o;
#pragma unroll
                                for (int r = 0; r < 4; r++) o[r] = (op_t)(acc[hA][hB][2 * g + h][j][r] + bv);
                                const int voff = voffV + ((t_s + fq * 8 >= P.S) ? wrap : 0);
                                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), rsV, voff, (int)((col + (unsigned)t_s) * 2u), F_STORE_AUX);
                                F_STORE_GUARD
                            }
                        }
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
    };
    // transposed part of a split launch: the accumulators hold V^T itself (rows = columns n of the launch, 8 consecutive key positions
    // per lane): row-major stores into the V^T image, bias per row, positions past the clip boundary move on by one clip
    auto store_vtT = [&](int m0, int n0) {
        typedef __attribute__((ext_vector_type(4))) op_t opx4;
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        const int clip0 = m0 / P.S, t_tile = m0 - clip0 * P.S;
        const int wrap = (Nv * P.vt_sp - P.S) * 2;
#pragma unroll
        for (int hB = 0; hB < 2; hB++) {
            const int t_g = t_tile + hB * 128 + wc * 32, rel = P.S - t_g;                      // wave-uniform: first position of the wave's 32, distance to the clip's end
            const bool cut = rel > 0 && rel < 32 && (rel & 7) == 4;                            // the boundary falls inside some lane's 8 positions
#pragma unroll
            for (int hA = 0; hA < 2; hA++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int n_r = hA * 128 + wr * 64 + i * 16;
                    const float bv = sbias[n0 + n_r + fr];
                    const unsigned base = (((unsigned)clip0 * (unsigned)Nv + (unsigned)(n0 - P.vt_n0 + n_r)) * (unsigned)P.vt_sp + (unsigned)t_g) * 2u;
                    if (!cut) {
                        opx8 o;
#pragma unroll
                        for (int e = 0; e < 8; e++) o[e] = (op_t)(acc[hA][hB][i][e >> 2][e & 3] + bv);
                        const int voff = voffV + ((t_g + fq * 8 >= P.S) ? wrap : 0);
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rsV, voff, (int)base, F_STORE_AUX);
                        F_STORE_GUARD
                    } else {
#pragma unroll
                        for (int h = 0; h < 2; h++) {
                            opx4 o;
#pragma unroll
                            for (int r = 0; r < 4; r++) o[r] = (op_t)(acc[hA][hB][i][h][r] + bv);
                            const int voff = voffV + h * 8 + ((t_g + fq * 8 + h * 4 >= P.S) ? wrap : 0);
                            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o), rsV, voff, (int)base, F_STORE_AUX);
                            F_STORE_GUARD
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
    };
    constexpr int EPI_OPS = 16;                              // vector-memory operations of the epilogue that sit in the vmcnt queue, AT LEAST (the V^T form issues one or
                                                             // two more when a clip boundary cuts a lane's 8 positions: the counted waits then wait for those too, which is safe)

    // ---- prologue: all of K-step 0, the first three half-tiles of K-step 1
    {
        FCursor c0; c0.kofs = 0; set_tile(c0, 0);
        it1 = 0; kt1 = 0; pc1 = c0; advance(pc1, it1, kt1);
        it2 = it1; kt2 = kt1; pc2 = pc1; advance(pc2, it2, kt2);
        __syncthreads();                                    // bias vector in LDS (before any DMA is in flight: this barrier drains)
        issue(c0, 0, 0); issue(c0, 1, 0); issue(c0, 2, 0); issue(c0, 3, 0);
        issue(pc1, 0, 1); issue(pc1, 1, 1); issue(pc1, 2, 1);
        f_wait_vm<6>();
        __builtin_amdgcn_s_barrier();
    }
    int c_m0, c_n0;
    S.tile(0, c_m0, c_n0);
    int par = 0;
#define F_GROUP(HA, HB, KK) __builtin_amdgcn_s_setprio(1); f_mma8<VT, HA, HB, KK>(acc, F);        \
                             __builtin_amdgcn_s_setprio(0); __builtin_amdgcn_sched_barrier(0);
#define F_ISSUE(C, KIND, PAR) __builtin_amdgcn_sched_barrier(0); issue(C, KIND, PAR); __builtin_amdgcn_sched_barrier(0);
    constexpr bool VT = EPI == FEPI_VT;                      // MFMA operand order (a split launch computes its transposed tiles as the transposed problem: same order)
    // K-step s (ring parity par), the ping-pong form of round 3: FOUR phases, each = [read this phase's new fragments out of LDS, stage one half-tile of a later
    // K-step, wait for the reads] barrier [16 MFMAs: one 64 x 32 quadrant over the whole K-step] barrier, and wave row 1 runs ONE BARRIER
    // BEHIND wave row 0 (an extra barrier before its first K-step, one for row 0 after its last): the two waves of a SIMD (w and w + 4) are
    // then always in opposite sections -- one owns the matrix pipe while the other issues its LDS reads and DMA and waits.  (In the
    // two-barrier form of rounds 2-3a both partners wanted the pipe at the same time and sat at the barrier / counted wait at the same time:
    // PMC, profiles/r03: waves 23 % issuing, 30 % parked, 48 % stalled at issue; pipe 58 % busy.)
    // Quadrant order (0,0) (0,1) (1,1) (1,0): phase 1 reads A-top + B-left (12 ds_read_b128), phase 2 B-right (4), phase 3 A-bottom (8, over
    // A-top's registers), phase 4 nothing (B-left is still in its registers).  Staging: phase 1 A-bottom(s+1), phase 2 A-top(s+2), phase 3
    // B-left(s+2), phase 4 B-right(s+2): a slot is re-staged at least one interval after BOTH rows read it (A-top and B-left are read in
    // phase 1, B-right in phase 2, A-bottom in phase 3) and every half-tile has 11 or more intervals to land.  One counted wait per
    // K-step, at the end of phase 4: all but the 6 youngest DMA instructions (= A-bottom(s+1) and everything older) have landed, which
    // covers every read of K-step s + 1; two barriers follow before the first of those reads.
    // after_stores: 1 = the first K-step after an epilogue (its 16+ stores sit in the in-order vmcnt queue behind the three half-tiles
    // K-step s + 1 reads first: the wait lets them and this K-step's 8 DMA instructions stay in flight), 2 = the second (A-bottom(s+1) was
    // staged after the stores: waited for at the end of phase 2, as late as its first read allows: the stores must have completed by then).
    auto kstep = [&](int after_stores) {
        f_read_A<0, 0>(F, dsm, ra, par); f_read_A<1, 0>(F, dsm, ra, par); f_read_B<0, 0>(F, dsm, rb, par); f_read_B<1, 0>(F, dsm, rb, par);
        F_ISSUE(pc1, 3, par ^ 1)
        f_wait_lgkm<0>();
        __builtin_amdgcn_s_barrier();
        F_GROUP(0, 0, 0) F_GROUP(0, 0, 1)
        __builtin_amdgcn_s_barrier();
        f_read_B<0, 1>(F, dsm, rb, par); f_read_B<1, 1>(F, dsm, rb, par);
        F_ISSUE(pc2, 0, par)
        if (after_stores == 2) f_wait_vm<10>();
        f_wait_lgkm<0>();
        __builtin_amdgcn_s_barrier();
        F_GROUP(0, 1, 0) F_GROUP(0, 1, 1)
        __builtin_amdgcn_s_barrier();
        f_read_A<0, 1>(F, dsm, ra, par); f_read_A<1, 1>(F, dsm, ra, par);
        F_ISSUE(pc2, 1, par)
        f_wait_lgkm<0>();
        __builtin_amdgcn_s_barrier();
        F_GROUP(1, 1, 0) F_GROUP(1, 1, 1)
        __builtin_amdgcn_s_barrier();
        F_ISSUE(pc2, 2, par)
        if (after_stores == 1) f_wait_vm<8 + EPI_OPS>(); else f_wait_vm<6>();
        __builtin_amdgcn_s_barrier();
        F_GROUP(1, 0, 0) F_GROUP(1, 0, 1)
        __builtin_amdgcn_s_barrier();
    };
    if (wr == 1) __builtin_amdgcn_s_barrier();
    for (int it = 0; it < S.my_tiles; it++) {
        const bool cur_vt = SPLIT ? (c_n0 >= P.vt_n0) : (EPI == FEPI_VT);            // workgroup-uniform
        for (int kt = 0; kt < nk; kt++) {
            const bool last = kt == nk - 1;
            kstep(it > 0 && nk >= 2 ? (kt == 0 ? 1 : kt == 1 ? 2 : 0) : 0);   // (a one-step K loop waits for its stores: plain counts)
            pc1 = pc2; it1 = it2; kt1 = kt2; advance(pc2, it2, kt2);
            if (last) {
                // the two wave rows write their halves of the tile AT THE SAME TIME: row 0 lets row 1 finish its last phase first (one extra
                // barrier), and row 1 falls one barrier behind again after the stores; left one barrier apart, each row's epilogue stood in an
                // interval of its own while the other row waited at the next barrier -- two epilogue times per tile instead of one
                if (wr == 0) __builtin_amdgcn_s_barrier();
                if constexpr (SPLIT) { if (cur_vt) store_vtT(c_m0, c_n0); else store_rm(c_m0, c_n0); }
                else if constexpr (EPI == FEPI_VT) store_vt(c_m0, c_n0, c_n0);
                else store_rm(c_m0, c_n0);
                // (starting the next tile from the zero CONSTANT instead -- v_mfma ..., 0 -- lets the register allocator place the fresh destination
                // on top of a dying A fragment; this multi-pass MFMA reads its sources while it already writes results: wrong values in a few lanes)
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++)
#pragma unroll
                        for (int i = 0; i < 4; i++)
#pragma unroll
                            for (int j = 0; j < 2; j++) acc[a][b][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (wr == 1) __builtin_amdgcn_s_barrier();
            }
            f_wait_lgkm<0>();
            par ^= 1;
        }
        if (it + 1 < S.my_tiles) S.tile(it + 1, c_m0, c_n0);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();
    f_wait_vm<0>();                                           // the surplus refills land before the workgroup (and its LDS allocation) ends
#undef F_GROUP
#undef F_ISSUE
#undef F_STORE_GUARD
}

// x = resid[row] + delta[row] (+ delta2[row]) (op_t branch outputs: attention projection, MLP), LayerNorm of x -> out; one wave per row.
// A layer makes two such passes: after the attention projection (x feeds ln2; the stream itself is NOT written back: the pass at
// the end of the layer re-derives it) and after the MLP (delta = the attention branch again, delta2 = the MLP branch: x =
// (resid + delta) + delta2, the same two roundings in the same order as writing the intermediate would give; x is written back).
// RIN / ROUT: the type the stream is read / written in.
//   float / float (bf16 operands, or fp16 operands with the fp32 stream): 8 + 14 bytes per element and layer;
//   op_t / op_t (round 4, fp16 operands with the 16-bit stream, PCE_OPERANDS_F16_RESID16): 6 + 10 bytes.  The reference's own arithmetic:
//     openai-whisper runs the model in half precision (transcribe's fp16=True behind Code/Aligners/use_whisper_timestamped.py:163), its
//     residual adds `x = x + self.attn(...)`, `x = x + self.mlp(...)` are fp16 + fp16 -> fp16 and only LayerNorm computes in fp32
//     (model.py LayerNorm.forward: super().forward(x.float()).type(x.dtype)).  Mirrored rounding for rounding: x1 = r16(x + delta) feeds
//     ln2 AS ROUNDED, x2 = r16(x1 + delta2) is the stream; both passes derive x1 the same way, so nothing depends on which pass ran;
//   float / op_t: the first layer of that mode (the convolution stem leaves gelu(conv2) + positional embedding in fp32: rounded on the way in).
template <class OUT, class RIN, class ROUT, int NV = 5>       // (NV: float4 per lane, as k_layernorm)
__global__ __launch_bounds__(256) void k_add_layernorm(const RIN *resid_in, ROUT *resid_out, const op_t *__restrict__ delta, const op_t *__restrict__ delta2,
                                                      int write_resid, const float *__restrict__ w,
                                                      const float *__restrict__ b, int64_t rows, int d, OUT *__restrict__ out, float eps,
                                                      op_t *__restrict__ out_bf16 = nullptr /* optional second copy of the output */)
{
    constexpr bool IN16 = !std::is_same<RIN, float>::value, OUT16 = !std::is_same<ROUT, float>::value;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    typedef __attribute__((ext_vector_type(4))) op_t opx4;
    const opx4 *dr = reinterpret_cast<const opx4 *>(delta + row * d);
    const opx4 *dr2 = reinterpret_cast<const opx4 *>(delta2 ? delta2 + row * d : nullptr);
    auto r16 = [](float x) -> float { return OUT16 ? (float)(op_t)x : x; };
    const int nv = d >> 2;
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int idx = lane + 64 * i;
        if (idx < nv) {
            // (read once / written once per pass: non-temporal, so that 3.5 GB of stream do not evict the next GEMM's weights from L2)
            f32x4 x;
            if constexpr (IN16) {
                const opx4 xh = __builtin_nontemporal_load(reinterpret_cast<const opx4 *>(resid_in + row * d) + idx);
                x = f32x4{(float)xh[0], (float)xh[1], (float)xh[2], (float)xh[3]};
            } else {
                x = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(resid_in + row * d) + idx);
                if constexpr (OUT16) x = f32x4{r16(x[0]), r16(x[1]), r16(x[2]), r16(x[3])};
            }
            const opx4 dl = __builtin_nontemporal_load(dr + idx);
            v[i] = make_float4(r16(x[0] + (float)dl[0]), r16(x[1] + (float)dl[1]), r16(x[2] + (float)dl[2]), r16(x[3] + (float)dl[3]));
            if (dr2) {
                const opx4 d2 = __builtin_nontemporal_load(dr2 + idx);
                v[i] = make_float4(r16(v[i].x + (float)d2[0]), r16(v[i].y + (float)d2[1]), r16(v[i].z + (float)d2[2]), r16(v[i].w + (float)d2[3]));
            }
            if (write_resid) {
                if constexpr (OUT16) {
                    opx4 o; o[0] = (op_t)v[i].x; o[1] = (op_t)v[i].y; o[2] = (op_t)v[i].z; o[3] = (op_t)v[i].w;
                    __builtin_nontemporal_store(o, reinterpret_cast<opx4 *>(resid_out + row * d) + idx);
                } else __builtin_nontemporal_store(f32x4{v[i].x, v[i].y, v[i].z, v[i].w}, reinterpret_cast<f32x4 *>(resid_out + row * d) + idx);
            }
        } else v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    s = wave_dpp_sum_f32(s);
    const float mean = s / (float)d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        if (lane + 64 * i < nv) {
            const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
            q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
        }
    }
    q = wave_dpp_sum_f32(q);
    const float inv = rsqrtf(q / (float)d + eps);
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int idx = lane + 64 * i;
        if (idx < nv) {
            const float4 ww = reinterpret_cast<const float4 *>(w)[idx], bb = reinterpret_cast<const float4 *>(b)[idx];
            const float y0 = (v[i].x - mean) * inv * ww.x + bb.x, y1 = (v[i].y - mean) * inv * ww.y + bb.y,
                        y2 = (v[i].z - mean) * inv * ww.z + bb.z, y3 = (v[i].w - mean) * inv * ww.w + bb.w;
            ln_store4<OUT>(out + row * d + 4 * idx, y0, y1, y2, y3);
            if (out_bf16) ln_store4<op_t>(out_bf16 + row * d + 4 * idx, y0, y1, y2, y3);
        }
    }
}

// k_add_layernorm with nothing to add: LayerNorm of the 16-bit stream as the FEPI_RESID epilogues left it (the two passes of a layer on the fused
// encoder path; no stream write).  The statistics are k_add_layernorm's, sum for sum.  One load of 8 bytes per lane in flight per wave left this
// pass latency-bound, so a wave takes LN0_ROWS consecutive rows and issues every load of them before the first use.
constexpr int LN0_ROWS = 2;
template <class OUT, int NV = 5>
__global__ __launch_bounds__(256) void k_add_layernorm0(const op_t *__restrict__ x, const float *__restrict__ w, const float *__restrict__ b, int64_t rows, int d,
                                                       OUT *__restrict__ out, float eps, op_t *__restrict__ out_bf16 = nullptr)
{
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * LN0_ROWS;
    const int lane = threadIdx.x & 63;
    if (row0 >= rows) return;
    typedef __attribute__((ext_vector_type(4))) op_t opx4;
    const int nv = d >> 2;
    opx4 raw[LN0_ROWS][NV];
    float4 ww[NV], bb[NV];                                                  // (read before the statistics too: a load between two rows' stores waits for the stores)
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int idx = lane + 64 * i;
        ww[i] = bb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < nv) { ww[i] = reinterpret_cast<const float4 *>(w)[idx]; bb[i] = reinterpret_cast<const float4 *>(b)[idx]; }
    }
#pragma unroll
    for (int r = 0; r < LN0_ROWS; r++) {
        const int64_t row = row0 + r < rows ? row0 + r : rows - 1;         // (a last odd row is read twice and written once)
#pragma unroll
        for (int i = 0; i < NV; i++) {
            const int idx = lane + 64 * i;
            raw[r][i] = opx4{(op_t)0.f, (op_t)0.f, (op_t)0.f, (op_t)0.f};
            if (idx < nv) raw[r][i] = __builtin_nontemporal_load(reinterpret_cast<const opx4 *>(x + row * d) + idx);
        }
    }
#pragma unroll
    for (int r = 0; r < LN0_ROWS; r++) {
        const int64_t row = row0 + r;
        if (row >= rows) break;
        float4 v[NV];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; i++) {
            v[i] = make_float4((float)raw[r][i][0], (float)raw[r][i][1], (float)raw[r][i][2], (float)raw[r][i][3]);
            s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
        }
        s = wave_dpp_sum_f32(s);
        const float mean = s / (float)d;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; i++) {
            if (lane + 64 * i < nv) {
                const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
                q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
        }
        q = wave_dpp_sum_f32(q);
        const float inv = rsqrtf(q / (float)d + eps);
#pragma unroll
        for (int i = 0; i < NV; i++) {
            const int idx = lane + 64 * i;
            if (idx < nv) {
                const float y0 = (v[i].x - mean) * inv * ww[i].x + bb[i].x, y1 = (v[i].y - mean) * inv * ww[i].y + bb[i].y,
                            y2 = (v[i].z - mean) * inv * ww[i].z + bb[i].z, y3 = (v[i].w - mean) * inv * ww[i].w + bb[i].w;
                ln_store4<OUT>(out + row * d + 4 * idx, y0, y1, y2, y3);
                if (out_bf16) ln_store4<op_t>(out_bf16 + row * d + 4 * idx, y0, y1, y2, y3);
            }
        }
    }
}
