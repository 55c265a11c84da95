// pce_gemm_tiled.inc -- the tiled GEMM kernels: k_gemm_bf16 (128 x 128), k_stem_fill, the few-row k_gemm_skinny, k_gemm_wide (128 x 256); included by
// pce_whisper_impl.inc inside its anonymous namespace, which holds their launchers (launch_gemm).
// ---------------------------------------------------------------------------
// GEMM  C[M x N] = A[M x K] * B[N x K]^T  (op_t in, fp32 accumulate)
// ---------------------------------------------------------------------------
enum { EPI_BF16 = 0, EPI_GELU_BF16 = 1, EPI_GELU_POS_F32 = 2, EPI_RESID_F32 = 3, EPI_QKV = 4, EPI_F32 = 5 };    // EPI_F32: C = A B^T + bias in fp32, C not read (the vocabulary logits)
constexpr int AT_SP = 1536;               // padded key axis of the transposed V image (multiple of the 64-key tile)
constexpr int G_BM = 128, G_BN = 128, G_BK = 64;
static_assert(G_BM == ST_TILE, "the stem's skip ranges count k_gemm_bf16 row tiles");

// GELU(x) = x/2 (1 + erf(x/sqrt 2)) = x/2 + |x|/2 erf(|x|/sqrt 2) (erf is odd: no sign select); erf by Abramowitz-Stegun 7.1.26,
// erf(z) = 1 - t P(t) exp(-z^2), t = 1/(1 + p z), |error| < 1.5e-7 -- far below the op_t step of the outputs (libm's erff costs more than
// the tile's MFMAs in a K = 768 epilogue).  With z' = z sqrt(log2 e) the exponential is a bare v_exp_f32 of -z'^2 and p z = (p / sqrt(log2 e)) z'.
// gelu_exact8 is the same operation sequence on eight values, written level by level: the eight dependency chains interleave, so the packed
// fp32 instructions the compiler forms need no wait states between them (the one-value form in a loop cost 18 issue slots per value, 4 of
// them s_nop; this costs 11).
constexpr float GELU_C = 0.70710678118654752440f * 1.2011224087864498f;     // |x| -> z' = |x| / sqrt 2 * sqrt(log2 e)
constexpr float GELU_P = 0.3275911f / 1.2011224087864498f;
__device__ __forceinline__ float gelu_exact(float x)
{
    const float zp = fabsf(x) * GELU_C;
    const float t = __builtin_amdgcn_rcpf(fmaf(zp, GELU_P, 1.0f));         // v_rcp_f32 (1 ulp); __frcp_rn expands to a 10-instruction IEEE division
    const float e = __builtin_amdgcn_exp2f(zp * -zp);
    const float poly = fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
    const float erf_abs = fmaf(-(t * poly), e, 1.0f);
    const float h = 0.5f * x;
    return fmaf(fabsf(h), erf_abs, h);
}
__device__ __forceinline__ void gelu_exact8(float (&x)[8])
{
    float zp[8], t[8], e[8], poly[8], h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) zp[i] = fabsf(x[i]) * GELU_C;
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = __builtin_amdgcn_rcpf(fmaf(zp[i], GELU_P, 1.0f));
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = __builtin_amdgcn_exp2f(zp[i] * -zp[i]);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = fmaf(t[i], 1.061405429f, -1.453152027f);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = fmaf(t[i], poly[i], 1.421413741f);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = fmaf(t[i], poly[i], -0.284496736f);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = fmaf(t[i], poly[i], 0.254829592f);
#pragma unroll
    for (int i = 0; i < 8; i++) poly[i] = t[i] * poly[i];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = fmaf(-poly[i], e[i], 1.0f);
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = 0.5f * x[i];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = fmaf(fabsf(h[i]), e[i], h[i]);
}

// LDS image of one operand tile: 128 rows x 64 op_t (128 B = eight 16-byte chunks per row), rows
// contiguous (what global_load_lds writes: wave-uniform base + lane * 16 B).  To keep the fragment
// reads (16 rows x one chunk per ds_read_b128 lane group) conflict-free the chunk index is
// XOR-swizzled with (row >> 1) & 7: applied to the GLOBAL source address when staging and to the
// LDS address when reading (the same involution on both sides).
__device__ __forceinline__ int swz_chunk(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

constexpr int G_THREADS = 512;
constexpr int G_TLD = G_BN + 4;           // fp32 epilogue tile row (pad keeps the accumulator scatter conflict-free)

// one operand tile (128 rows x 64 k): 16 wave-instructions of 1 KiB (8 rows each); 8 waves -> 2 each
__device__ __forceinline__ void stage_tile(const op_t *__restrict__ G, int64_t ld, int row0, int row_max, int k0, op_t *lds_tile, int wv, int lane)
{
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int r0 = wv * 16 + i * 8;
        const int row = r0 + (lane >> 3);
        const int c = swz_chunk(row, lane & 7);
        int gr = row0 + row; if (gr > row_max) gr = row_max;
        const op_t *src = G + (int64_t)gr * ld + k0 + c * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(lds_tile + r0 * G_BK), 16, 0, 0);
    }
}

template <int EPI>
__device__ __forceinline__ void gemm_fetch_bias(const float *__restrict__ bias, int n0, int tid, float (&bv)[8], float &bv_col)
{
    constexpr bool OUT_BF16 = (EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_QKV);
    const int cx0 = OUT_BF16 ? (tid & 15) * 8 : (tid & 31) * 4;
#pragma unroll
    for (int e = 0; e < 8; e++) bv[e] = (bias && e < (OUT_BF16 ? 8 : 4)) ? bias[n0 + cx0 + e] : 0.f;
    bv_col = (EPI == EPI_QKV && bias) ? bias[n0 + (tid & 127)] : 0.f;      // transposed-V path: one column per thread
}

// Output stage shared by the GEMM kernels: a [128][G_TLD] fp32 tile in LDS (rows m0.., columns n0..) leaves as full
// 256-byte row segments with the fused bias / GELU / positional add / residual accumulate / transposed-V write.
// bv / bv_col: this thread's bias values for the tile's columns, fetched by the caller before its K loop.
template <int EPI>
__device__ __forceinline__ void gemm_store_tile(const float *tile, int tid, int m0, int n0, int M, int N, const float (&bv)[8], float bv_col,
                                                void *__restrict__ Cv, int64_t ldc, int64_t cbase, const float *__restrict__ pos, int pos_T,
                                                int v_col0, int vt_sp, float *__restrict__ rep = nullptr, int rep_row = 0)
{
    if (EPI == EPI_QKV && n0 >= v_col0) {
        // V columns: written transposed, vt[clip][head][d][key], so the attention kernel can stage V^T tiles
        // (8 keys contiguous per d) without an LDS transpose.  `pos` carries the vt pointer, pos_T = S.
        op_t *vt = reinterpret_cast<op_t *>(const_cast<float *>(pos));
        const int dmodel = N - v_col0, S = pos_T;                   // V is the last d_model columns
        const int cc = tid & 127, rg = tid >> 7;                  // one column, 8-row groups
        const int n = n0 + cc - v_col0, head = n >> 6, dd = n & 63;
        const float bv = bv_col;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = rg * 8 + 32 * p;
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {                      // halves of 4 tokens never straddle a clip (S % 4 == 0)
                const int m = m0 + row + 4 * hf;
                if (m >= M) continue;
                const int clip = m / S, t = m - clip * S;
                typedef __attribute__((ext_vector_type(4))) op_t opx4;
                opx4 o;
#pragma unroll
                for (int e = 0; e < 4; e++) o[e] = (op_t)(tile[(row + 4 * hf + e) * G_TLD + cc] + bv);
                *reinterpret_cast<opx4 *>(vt + (((int64_t)clip * (dmodel >> 6) + head) * 64 + dd) * vt_sp + t) = o;
            }
        }
    } else if (EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_QKV) {
        // 16 threads x 8 columns per row, 32 rows per pass
        const int cx = (tid & 15) * 8, ry = tid >> 4;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = ry + 32 * p;
            if (m0 + row >= M) continue;
            const float4 v0 = *reinterpret_cast<const float4 *>(&tile[row * G_TLD + cx]);
            const float4 v1 = *reinterpret_cast<const float4 *>(&tile[row * G_TLD + cx + 4]);
            const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
            opx8 o;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float t = v[e] + bv[e];
                o[e] = (op_t)(EPI == EPI_GELU_BF16 ? gelu_exact(t) : t);
            }
            // written once, read by the next kernel: keep it out of the way of the operand tiles in L2
            __builtin_nontemporal_store(o, reinterpret_cast<opx8 *>(reinterpret_cast<op_t *>(Cv) + cbase + (int64_t)(m0 + row) * ldc + n0 + cx));
        }
    } else {
        // fp32 outputs: 32 threads x 4 columns per row, 16 rows per pass
        const int cx = (tid & 31) * 4, ry = tid >> 5;
        float4 oldv[8];
        if (EPI == EPI_RESID_F32) {
#pragma unroll
            for (int p = 0; p < 8; p++) {                         // all eight residual loads in flight together
                const int row = ry + 16 * p;
                oldv[p] = m0 + row < M ? *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(Cv) + cbase + (int64_t)(m0 + row) * ldc + n0 + cx)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int p = 0; p < 8; p++) {
            const int row = ry + 16 * p;
            if (m0 + row >= M) continue;
            const float4 v = *reinterpret_cast<const float4 *>(&tile[row * G_TLD + cx]);
            float4 *dst = reinterpret_cast<float4 *>(reinterpret_cast<float *>(Cv) + cbase + (int64_t)(m0 + row) * ldc + n0 + cx);
            float4 o;
            if (EPI == EPI_GELU_POS_F32) {
                // (conv2 of the stem) the accumulators of the row whose output the skipped rows repeat: k_stem_fill finishes them with the expression below
                if (rep && m0 + row == rep_row) *reinterpret_cast<float4 *>(rep + n0 + cx) = v;
                const float4 pe = *reinterpret_cast<const float4 *>(pos + (int64_t)((m0 + row) % pos_T) * N + n0 + cx);
                o = make_float4(gelu_exact(v.x + bv[0]) + pe.x, gelu_exact(v.y + bv[1]) + pe.y, gelu_exact(v.z + bv[2]) + pe.z,
                                gelu_exact(v.w + bv[3]) + pe.w);
            } else {
                const float4 old = EPI == EPI_RESID_F32 ? oldv[p] : make_float4(0.f, 0.f, 0.f, 0.f);      // (0 + v is v: the bits of the former cleared-C form)
                o = make_float4(old.x + v.x + bv[0], old.y + v.y + bv[1], old.z + v.z + bv[2], old.w + v.w + bv[3]);
            }
            *dst = o;
        }
    }
}

// 8 wavefronts as 2 (M) x 4 (N), each owning a 64 x 32 slice of the 128 x 128 tile.  Three LDS stages:
// while tile kt is multiplied, tiles kt+1 and kt+2 are in flight as LDS-DMA (4 instructions per wave and
// tile), so a tile has two full K-steps to arrive.  The barrier is a raw s_barrier behind a COUNTED
// s_waitcnt vmcnt(4): __syncthreads() would drain the DMA queue (vmcnt(0)) and serialise the ring.
// G_STAGES = 2: two workgroups per CU cover each other's waits (big grids).  G_STAGES = 4 (round 3): the few-row launches of an
// incremental decoding step (M = clips: 2 x N/128 workgroups on 256 CUs) are alone on their CU and each K-step waited out a full
// L2 / HBM round trip (12 K-steps x 1.5 us = the 24 us such a launch took); with three tiles in flight the K loop runs at the
// DMA issue rate instead.
template <int EPI, int G_STAGES = 2>
__global__ __launch_bounds__(G_THREADS, G_STAGES == 2 ? 4 : 2) void k_gemm_bf16(const op_t *__restrict__ A, int64_t lda, int64_t a_batch,
                                                        const op_t *__restrict__ B, int M, int N, int K,
                                                        const float *__restrict__ bias, void *__restrict__ Cv, int64_t ldc, int64_t c_batch,
                                                        const float *__restrict__ pos, int pos_T, int v_col0, int vt_sp, int sn_tiles, int sm_tiles,
                                                        GemmSkip skip)
{
    // operand ring [stage][A|B][128][64] op_t, re-used as the fp32 epilogue tile [128][G_TLD]
    constexpr int SMEM_ELEMS = (G_STAGES * 2 * G_BM * G_BK * 2 > G_BM * G_TLD * 4 ? G_STAGES * 2 * G_BM * G_BK : G_BM * G_TLD * 2);
    __shared__ __attribute__((aligned(1024))) op_t smem[SMEM_ELEMS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = wv >> 2, wc = wv & 3;
    // XCD-aware, L2-sized tile order.  Workgroups go to the 8 XCDs round-robin, so XCD x is given a contiguous range of
    // the tile sequence, and the ~64 workgroups resident on an XCD at a time are 64 consecutive tiles of it.  The
    // sequence walks SUPERTILES of sm (M) x sn (N) tiles: their operands (sm A row blocks + sn B row blocks of 128 x K)
    // fit the XCD's 4 MB L2 and every block is re-read 8 times from it.  (A plain row-major sequence keeps 2-3 A blocks
    // and ALL of B live: at N = 3072 that is 4.7 MB of weights, which evicts itself; measured L2 hit rate 50 %.)
    const int tiles_n = (int)gridDim.x, tiles_m_pad = (int)gridDim.y;          // gridDim.y is padded to a multiple of 8
    int lin = (int)blockIdx.y * tiles_n + (int)blockIdx.x;
    const int total = tiles_n * tiles_m_pad;
    // With a skip description the XCD's range rotates with the batch entry: every entry skips the SAME stretch of the sequence (a 10 s clip: conv2's row
    // tiles 4-10 beside the grid's padding tiles 12-15), and un-rotated the XCDs that own that stretch idle through the whole launch while two of them carry
    // all the work (measured: 58 % of the tiles skipped, 6 % of the time).  Which workgroup computes a tile does not change the tile.
    if ((total & 7) == 0) lin = (((lin & 7) + (skip.tiles ? (int)blockIdx.z : 0)) & 7) * (total >> 3) + (lin >> 3);
    int m0, n0;
    {
        const int per = sm_tiles * sn_tiles, sup = lin / per, r = lin - sup * per;
        const int n_sn = tiles_n / sn_tiles;
        const int tm = (sup / n_sn) * sm_tiles + r / sn_tiles, tn = (sup % n_sn) * sn_tiles + r % sn_tiles;
        m0 = tm * G_BM; n0 = tn * G_BN;
        if (m0 >= M) return;                                                     // padding tile
        if (skip.tiles) {                                                        // a tile this batch entry does not need (the conv stem: rows of the zero padding)
            const int2 sk = skip.tiles[blockIdx.z];
            if (tm >= sk.x && tm <= sk.y) return;
        }
    }
    // the epilogue's bias values are fetched now: after the K loop their load latency (1-2 us) was fully exposed
    float bv[8]; float bv_col;
    gemm_fetch_bias<EPI>(bias, n0, tid, bv, bv_col);
    A += (int64_t)blockIdx.z * a_batch;
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    const int nk = K / G_BK;
    constexpr int STAGE = 2 * G_BM * G_BK;
    // prologue: tiles 0 .. G_STAGES - 2 (every tile is 4 DMA instructions per wave; a tile past the end of K is issued anyway -- the last
    // tile again, into a slot nobody reads -- so that the counted waits below are the same in every iteration)
#pragma unroll
    for (int t = 0; t < G_STAGES - 1; t++) {
        const int tt = t < nk ? t : nk - 1;
        stage_tile(A, lda, m0, M - 1, tt * G_BK, smem + t * STAGE, wv, lane);
        stage_tile(B, K, n0, N - 1, tt * G_BK, smem + t * STAGE + G_BM * G_BK, wv, lane);
    }
    for (int kt = 0; kt < nk; kt++) {
        const op_t *sA = smem + (kt % G_STAGES) * STAGE, *sB = sA + G_BM * G_BK;
        // tile kt has landed once at most the DMAs of the G_STAGES - 2 younger tiles of this wave are outstanding
        __builtin_amdgcn_s_waitcnt(0x0F70 | (((4 * (G_STAGES - 2)) >> 4) << 14) | ((4 * (G_STAGES - 2)) & 15));
        __builtin_amdgcn_s_barrier();
        if (G_STAGES > 2 || kt + G_STAGES - 1 < nk) {        // refill the stage tile kt-1 has just released (deep ring: always, see the prologue)
            const int tn = kt + G_STAGES - 1 < nk ? kt + G_STAGES - 1 : nk - 1;
            op_t *nA = smem + ((kt + G_STAGES - 1) % G_STAGES) * STAGE;
            stage_tile(A, lda, m0, M - 1, tn * G_BK, nA, wv, lane);
            stage_tile(B, K, n0, N - 1, tn * G_BK, nA + G_BM * G_BK, wv, lane);
        }
#pragma unroll
        for (int kk = 0; kk < G_BK; kk += 32) {
            opx8 a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = wr * 64 + i * 16 + fr;
                a[i] = *reinterpret_cast<const opx8 *>(&sA[row * G_BK + swz_chunk(row, (kk >> 3) + fq) * 8]);
            }
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int row = wc * 32 + j * 16 + fr;
                b[j] = *reinterpret_cast<const opx8 *>(&sB[row * G_BK + swz_chunk(row, (kk >> 3) + fq) * 8]);
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
        }
    }
    // epilogue.  The accumulator layout (col = lane & 15, row = (lane >> 4) * 4 + reg) would store 2-byte
    // elements 32 B at a time; measured, such an epilogue cost more than the whole K loop.  The tile
    // goes through LDS instead (the operand ring is free now) and leaves as full 256-B row segments.
    if (G_STAGES > 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the surplus refills of the deep ring must have landed before the ring is reused
    __builtin_amdgcn_s_barrier();                           // every wave is done reading the operand stages
    float *tile = reinterpret_cast<float *>(smem);           // [128][G_TLD] fp32 = 66 KiB
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                tile[(wr * 64 + i * 16 + fq * 4 + r) * G_TLD + wc * 32 + j * 16 + fr] = acc[i][j][r];
    __syncthreads();
    gemm_store_tile<EPI>(tile, tid, m0, n0, M, N, bv, bv_col, Cv, ldc, (int64_t)blockIdx.z * c_batch, pos, pos_T, v_col0, vt_sp,
                         skip.rep ? skip.rep + (int64_t)blockIdx.z * N : nullptr, skip.rep_row);
}

// k_stem_fill: the conv2 rows k_gemm_bf16 skipped (GemmSkip).  Rows [ST_TILE s, ST_TILE ST_C2_LAST) of clip blockIdx.y, s = tiles[clip].x, have the
// accumulators of the row the last tile left in rep[clip][d]; what differs is the positional row.  The expression is EPI_GELU_POS_F32's, so the bits are.
constexpr int SF_ROWS = 16;                                   // rows per workgroup (divides ST_TILE: a workgroup is skipped rows only, or none)
static_assert(ST_TILE % SF_ROWS == 0, "a fill workgroup must not straddle a tile boundary");
__global__ __launch_bounds__(256) void k_stem_fill(const int2 *__restrict__ tiles, const float *__restrict__ rep, const float *__restrict__ bias,
                                                   const float *__restrict__ pos /* [W_CTX][d] */, int d /* % 4 == 0 */, float *__restrict__ out /* [clip][W_CTX][d] */)
{
    const int clip = blockIdx.y, t0 = blockIdx.x * SF_ROWS;
    if (t0 < tiles[clip].x * ST_TILE || t0 >= ST_C2_LAST * ST_TILE) return;
    const int d4 = d >> 2;
    const float *acc = rep + (int64_t)clip * d;
    float *dst = out + ((int64_t)clip * W_CTX + t0) * d;
    const float *pe0 = pos + (int64_t)t0 * d;
    for (int i = threadIdx.x; i < SF_ROWS * d4; i += 256) {
        const int cx = (i % d4) * 4;
        const float4 v = *reinterpret_cast<const float4 *>(acc + cx), b = *reinterpret_cast<const float4 *>(bias + cx);
        const float4 pe = *reinterpret_cast<const float4 *>(pe0 + (int64_t)i * 4);
        const float4 o = make_float4(gelu_exact(v.x + b.x) + pe.x, gelu_exact(v.y + b.y) + pe.y, gelu_exact(v.z + b.z) + pe.z, gelu_exact(v.w + b.w) + pe.w);
        *reinterpret_cast<float4 *>(dst + (int64_t)i * 4) = o;
    }
}

// ---------------------------------------------------------------------------
// k_gemm_skinny (round 3): the projections of an incremental decoding step, C[M][N] with M = the number of sequences (a few hundred rows)
// and N, K <= a few thousand.  Such a launch is a LATENCY chain, not a throughput problem: the 128 x 128 kernel puts 2 x N/128
// workgroups on 256 CUs and each walks K in 64-deep steps (10-26 us per launch, 74 launches per decoding step).  Here a workgroup
// owns 64 rows x 32 columns (M/64 x N/32 workgroups: 96 for a 768-wide projection of 256 rows) and streams K in 256-deep chunks
// through three LDS buffers (48 KB each: 64 + 32 rows of 512 B), two chunks ahead: a K = 768 product has ALL its operand bytes in
// flight before the first MFMA (one memory round trip), K = 3072 keeps 96 KB per CU in flight.  4 waves, 16 rows x 32 columns
// each, accumulators stored straight from registers (a tile is 8 KB: no LDS pass).
// ---------------------------------------------------------------------------
constexpr int S_BM = 64, S_BN = 32, S_KC = 256, S_THREADS = 256, S_NBUF = 3;
constexpr int S_BUF = (S_BM + S_BN) * S_KC;                       // elements per buffer (48 KB)
constexpr int S_LDS = S_NBUF * S_BUF * 2;                          // dynamic LDS of a launch (bytes)
__device__ __forceinline__ int swz512(int row, int chunk) { return chunk ^ (row & 15); }     // 512-byte rows: 32 chunks, the low four bits swizzled
template <int EPI>
__global__ __launch_bounds__(S_THREADS) void k_gemm_skinny(const op_t *__restrict__ A, int64_t lda, const op_t *__restrict__ B, int M, int N, int K,
                                                           const float *__restrict__ bias, void *__restrict__ Cv, int64_t ldc)
{
    extern __shared__ __attribute__((aligned(1024))) op_t sk[];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.x * S_BN, m0 = blockIdx.y * S_BM;
    const int nk = K / S_KC;
    // one chunk = 96 rows of 512 B = 48 wave-instructions of 2 rows; wave w issues instructions w, w + 4, ... (12 each)
    auto stage = [&](int kc, int buf) {
        op_t *dst = sk + buf * S_BUF;
#pragma unroll
        for (int i = 0; i < 12; i++) {
            const int inst = wv + 4 * i, row = inst * 2 + (lane >> 5);               // LDS row 0..95: 0..63 = A, 64..95 = B
            const int c = swz512(row, lane & 31);
            const op_t *src;
            if (row < S_BM) { int gr = m0 + row; if (gr > M - 1) gr = M - 1; src = A + (int64_t)gr * lda + kc * S_KC + c * 8; }
            else { int gr = n0 + row - S_BM; if (gr > N - 1) gr = N - 1; src = B + (int64_t)gr * K + kc * S_KC + c * 8; }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(dst + inst * 2 * S_KC), 16, 0, 0);
        }
    };
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    // The products are formed TRANSPOSED (weights as the A operand, activations as B: D[column][row]), so a lane ends up with four CONSECUTIVE
    // columns 4 fq .. 4 fq + 3 of ONE row (wave row fr) per 16-column block: the tile leaves as 8- / 16-byte stores (and the old residual values
    // arrive as 16-byte loads) instead of four 2- / 4-byte ones per block -- the same sums in the same order, the same bits.
    // the epilogue's bias values now: their latency hides behind the operand stream (the counted waits below retire them first)
    const int e_row = m0 + wv * 16 + fr;
    f32x4 bvec[2];
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) { const int col = n0 + j * 16 + fq * 4 + r; bvec[j][r] = (bias && col < N) ? bias[col] : 0.f; }
    // ... and, for the accumulate-into-the-residual epilogue, the old values of C (round 5: fetched after the K loop they were a second,
    // fully exposed memory round trip of every out-projection / fc2 launch)
    f32x4 old_c[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (EPI == EPI_RESID_F32) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int col = n0 + j * 16 + fq * 4;
            if (e_row < M && col + 3 < N) old_c[j] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const float *>(Cv) + (int64_t)e_row * ldc + col);
            else if (e_row < M)
#pragma unroll
                for (int r = 0; r < 4; r++) if (col + r < N) old_c[j][r] = reinterpret_cast<const float *>(Cv)[(int64_t)e_row * ldc + col + r];
        }
    }
    // K <= 3 chunks (every projection of a decoding step but fc2): the whole product is in flight before the first MFMA -- ONE memory round
    // trip; longer K keeps two chunks ahead.  (A chunk past the end is issued anyway, into a buffer nobody reads, so that the counted waits
    // are the same in every iteration.)
    const bool all_up_front = nk <= S_NBUF;
#pragma unroll
    for (int t = 0; t < S_NBUF - 1; t++) stage(t < nk ? t : nk - 1, t);
    if (all_up_front) stage(nk - 1, S_NBUF - 1);                 // chunk 2 of a three-chunk product (a shorter one: its last chunk again, unread)
    for (int kc = 0; kc < nk; kc++) {
        // chunk kc has landed once at most the DMA instructions of the younger chunks are outstanding in this wave
        if (all_up_front) {
            if (kc == 0) __builtin_amdgcn_s_waitcnt(0x0F70 | (((24) >> 4) << 14) | ((24) & 15));
            else if (kc == 1) __builtin_amdgcn_s_waitcnt(0x0F70 | 12);
            else __builtin_amdgcn_s_waitcnt(0x0F70 | 0);
            __builtin_amdgcn_s_barrier();
        } else {
            __builtin_amdgcn_s_waitcnt(0x0F70 | 12);
            __builtin_amdgcn_s_barrier();
            const int tn = kc + S_NBUF - 1; stage(tn < nk ? tn : nk - 1, tn % S_NBUF);
        }
        const op_t *sA = sk + (kc % S_NBUF) * S_BUF, *sB = sA + S_BM * S_KC;
#pragma unroll
        for (int ks = 0; ks < S_KC / 32; ks++) {
            const int ra = wv * 16 + fr;
            const opx8 a = *reinterpret_cast<const opx8 *>(&sA[ra * S_KC + swz512(ra, ks * 4 + fq) * 8]);
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int rb = j * 16 + fr;                                       // (LDS row 64 + rb: (64 + rb) & 15 == rb & 15)
                const opx8 b = *reinterpret_cast<const opx8 *>(&sB[rb * S_KC + swz512(rb, ks * 4 + fq) * 8]);
                acc[j] = mfma16(b, a, acc[j]);                                    // (transposed: see above)
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the surplus refills land before the wave (and its LDS allocation) ends
    // D layout of the transposed 16 x 16 product: activation row = lane & 15, columns (lane >> 4) * 4 + register
    if (e_row >= M) return;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int col = n0 + j * 16 + fq * 4;
        float t[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // (the same association as the tiled kernels' epilogues -- (old + sum) + bias -- so that a row's bits do not depend on which kernel its batch size selects)
            if (EPI == EPI_RESID_F32) t[r] = (old_c[j][r] + acc[j][r]) + bvec[j][r];
            else { const float v = acc[j][r] + bvec[j][r]; t[r] = EPI == EPI_GELU_BF16 ? gelu_exact(v) : v; }
        }
        if (col + 3 < N) {
            if (EPI == EPI_RESID_F32) *reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(Cv) + (int64_t)e_row * ldc + col) = f32x4{t[0], t[1], t[2], t[3]};
            else {
                typedef __attribute__((ext_vector_type(4))) op_t opx4;
                *reinterpret_cast<opx4 *>(reinterpret_cast<op_t *>(Cv) + (int64_t)e_row * ldc + col) = opx4{(op_t)t[0], (op_t)t[1], (op_t)t[2], (op_t)t[3]};
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (col + r < N) {
                    if (EPI == EPI_RESID_F32) reinterpret_cast<float *>(Cv)[(int64_t)e_row * ldc + col + r] = t[r];
                    else reinterpret_cast<op_t *>(Cv)[(int64_t)e_row * ldc + col + r] = (op_t)t[r];
                }
        }
    }
}

// ---------------------------------------------------------------------------
// 128 x 256 tile variant for wide outputs (N >= 2048: QKV, fc1).  Skipping the A-operand loads of the 128 x 128 kernel
// speeds the encoder up by 36 %, skipping the B loads by 12 % (ablation): the ACTIVATION stream is what these launches
// wait for.  A tile twice as wide reads every A row block half as often; the weights (B) stay L2-resident anyway.
// 8 waves as 2 (M) x 4 (N), 64 x 64 per wave, 32-deep K-steps (16 MFMAs per wave between barriers, as before), two
// 24 KB stages so that two workgroups still share a CU, and the output leaves through the same 128 x 128 LDS tile
// in two column passes.
// ---------------------------------------------------------------------------
constexpr int W_BN = 256, W_BK = 32, W_STAGES = 2;   // a third stage (72 KB, still two workgroups per CU) measured +0.2 %: not latency bound
constexpr int W_STAGE = (G_BM + W_BN) * W_BK;                   // op_t elements per stage (24 KB)
// 64-byte rows (see swz_chunk).  A ds_read_b128 is serviced in four groups of sixteen lanes that are NOT lane-contiguous ({0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31}, ...: MI355X_MICROARCH.md, LDS): a fragment read (lane = 16 k-chunk + row) puts rows 0-3 and 12-15 of one chunk and
// rows 4-11 of the next into one group.  chunk ^ (row >> 2) left them two to a bank (SQ_LDS_BANK_CONFLICT 44 % of the LDS cycles of
// k_gemm_wide); chunk ^ (-(row >> 2) & 3) gives every lane of a group its own 16 bytes of the 256-byte bank row.
__device__ __forceinline__ int swz32(int row, int chunk) { return chunk ^ ((-(row >> 2)) & 3); }
// ROWS x 32 k operand tile: wave-instructions of 1 KiB (16 rows each)
template <int ROWS>
__device__ __forceinline__ void stage_rows32(const op_t *__restrict__ G, int64_t ld, int row0, int row_max, int k0, op_t *lds_tile, int wv, int lane)
{
#pragma unroll
    for (int i = 0; i < ROWS / 128; i++) {
        const int r0 = (wv + 8 * i) * 16;
        const int row = r0 + (lane >> 2);
        const int c = swz32(row, lane & 3);
        int gr = row0 + row; if (gr > row_max) gr = row_max;
        const op_t *src = G + (int64_t)gr * ld + k0 + c * 8;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(lds_tile + r0 * W_BK), 16, 0, 0);
    }
}

template <int EPI>
__global__ __launch_bounds__(G_THREADS, 4) void k_gemm_wide(const op_t *__restrict__ A, int64_t lda, int64_t a_batch,
                                                        const op_t *__restrict__ B, int M, int N, int K,
                                                        const float *__restrict__ bias, void *__restrict__ Cv, int64_t ldc, int64_t c_batch,
                                                        const float *__restrict__ pos, int pos_T, int v_col0, int vt_sp, int sn_tiles, int sm_tiles)
{
    constexpr int SMEM_ELEMS = (W_STAGES * W_STAGE * 2 > G_BM * G_TLD * 4 ? W_STAGES * W_STAGE : G_BM * G_TLD * 2);
    __shared__ __attribute__((aligned(1024))) op_t smem[SMEM_ELEMS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = wv >> 2, wc = wv & 3;                         // 2 x 4 waves, 64 x 64 each
    const int tiles_n = (int)gridDim.x, tiles_m_pad = (int)gridDim.y;
    int lin = (int)blockIdx.y * tiles_n + (int)blockIdx.x;
    const int total = tiles_n * tiles_m_pad;
    if ((total & 7) == 0) lin = (lin & 7) * (total >> 3) + (lin >> 3);
    int m0, n0;
    {
        const int per = sm_tiles * sn_tiles, sup = lin / per, r = lin - sup * per;
        const int n_sn = tiles_n / sn_tiles;
        const int tm = (sup / n_sn) * sm_tiles + r / sn_tiles, tn = (sup % n_sn) * sn_tiles + r % sn_tiles;
        m0 = tm * G_BM; n0 = tn * W_BN;
        if (m0 >= M) return;
    }
    float bv0[8], bv1[8]; float bc0, bc1;
    gemm_fetch_bias<EPI>(bias, n0, tid, bv0, bc0);
    gemm_fetch_bias<EPI>(bias, n0 + 128, tid, bv1, bc1);
    A += (int64_t)blockIdx.z * a_batch;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fq = lane >> 4;
    const int nk = K / W_BK;
    // the bias loads above are older than every DMA: a counted wait on the DMAs retires them too
#pragma unroll
    for (int s = 0; s < W_STAGES - 1; s++)
        if (s < nk) {
            stage_rows32<G_BM>(A, lda, m0, M - 1, s * W_BK, smem + s * W_STAGE, wv, lane);
            stage_rows32<W_BN>(B, K, n0, N - 1, s * W_BK, smem + s * W_STAGE + G_BM * W_BK, wv, lane);
        }
    int cur = 0;
    for (int kt = 0; kt < nk; kt++) {
        const op_t *sA = smem + cur * W_STAGE, *sB = sA + G_BM * W_BK;
        // K-step kt has landed once at most the DMAs of the one younger stage (3 per wave) are outstanding
        if (W_STAGES > 2 && kt + 1 < nk) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + W_STAGES - 1 < nk) {                            // refill the stage K-step kt-1 has released
            int nx = cur + W_STAGES - 1; if (nx >= W_STAGES) nx -= W_STAGES;
            op_t *nA = smem + nx * W_STAGE;
            stage_rows32<G_BM>(A, lda, m0, M - 1, (kt + W_STAGES - 1) * W_BK, nA, wv, lane);
            stage_rows32<W_BN>(B, K, n0, N - 1, (kt + W_STAGES - 1) * W_BK, nA + G_BM * W_BK, wv, lane);
        }
        opx8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int row = wr * 64 + i * 16 + fr;
            a[i] = *reinterpret_cast<const opx8 *>(&sA[row * W_BK + swz32(row, fq) * 8]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int row = wc * 64 + j * 16 + fr;
            b[j] = *reinterpret_cast<const opx8 *>(&sB[row * W_BK + swz32(row, fq) * 8]);
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = mfma16(a[i], b[j], acc[i][j]);
        cur = cur + 1 == W_STAGES ? 0 : cur + 1;
    }
    float *tile = reinterpret_cast<float *>(smem);               // [128][G_TLD] fp32: one half of the columns per pass
#pragma unroll
    for (int p = 0; p < 2; p++) {
        __syncthreads();                                         // operand reads (p = 0) / the first pass's tile reads are done
        if ((wc >> 1) == p) {
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        tile[(wr * 64 + i * 16 + fq * 4 + r) * G_TLD + (wc & 1) * 64 + j * 16 + fr] = acc[i][j][r];
        }
        __syncthreads();
        if (p == 0) gemm_store_tile<EPI>(tile, tid, m0, n0, M, N, bv0, bc0, Cv, ldc, (int64_t)blockIdx.z * c_batch, pos, pos_T, v_col0, vt_sp);
        else gemm_store_tile<EPI>(tile, tid, m0, n0 + 128, M, N, bv1, bc1, Cv, ldc, (int64_t)blockIdx.z * c_batch, pos, pos_T, v_col0, vt_sp);
    }
}
