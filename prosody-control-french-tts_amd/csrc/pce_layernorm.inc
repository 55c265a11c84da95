// pce_layernorm.inc -- k_layernorm (included by pce_whisper_impl.inc inside its anonymous namespace; the residual-adding forms are in pce_gemm256.inc).
// ---------------------------------------------------------------------------
// LayerNorm over the last dimension (one wavefront per row)
// ---------------------------------------------------------------------------
// The row is read once with 16-byte loads and kept in registers: NV float4 per lane, so d <= 256 NV.  NV = 5 up to d = 1280 (every width of
// the Whisper / BERT checkpoints: the code and bits that k_xq_fused restates), NV = 8 up to LN_D_MAX; launch_layernorm and launch_add_layernorm
// pick it from d.  Statistics in fp32, two-pass (mean, then centred second moment) as torch does.
template <class OUT> __device__ __forceinline__ void ln_store4(OUT *p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void ln_store4<float>(float *p, float a, float b, float c, float d)
{
    *reinterpret_cast<float4 *>(p) = make_float4(a, b, c, d);
}
template <> __device__ __forceinline__ void ln_store4<op_t>(op_t *p, float a, float b, float c, float d)
{
    typedef __attribute__((ext_vector_type(4))) op_t opx4;
    opx4 v; v[0] = (op_t)a; v[1] = (op_t)b; v[2] = (op_t)c; v[3] = (op_t)d;
    *reinterpret_cast<opx4 *>(p) = v;
}

constexpr int LN_D_MAX = 2048;
template <class OUT, int NV = 5>
__global__ __launch_bounds__(256) void k_layernorm(const float *x, const float *__restrict__ w, const float *__restrict__ b,
                                                  int64_t rows, int d, OUT *__restrict__ out, float eps = 1e-5f, float *out2 = nullptr, int round_in16 = 0,
                                                  op_t *__restrict__ in16_out = nullptr)
{   // out2 (optional, may alias x): the same values in fp32 -- the post-LN residual stream of the BERT layers
    // round_in16: the input is taken as rounded to op_t (the first LayerNorm of the encoder in the 16-bit-stream mode: the reference's stem output
    // IS fp16 -- gelu(conv2) + positional embedding in half precision -- and k_add_layernorm's first-layer form rounds the same values the same way)
    // in16_out (with round_in16): the rounded input itself, as op_t rows -- the 16-bit residual stream the GEMM epilogues of layer 0 add to
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float4 *xr = reinterpret_cast<const float4 *>(x + row * d);
    const int nv = d >> 2;                               // float4 per row, d % 4 == 0
    float4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const int idx = lane + 64 * i;
        v[i] = idx < nv ? xr[idx] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (round_in16) v[i] = make_float4((float)(op_t)v[i].x, (float)(op_t)v[i].y, (float)(op_t)v[i].z, (float)(op_t)v[i].w);
        if (in16_out && idx < nv) ln_store4<op_t>(in16_out + row * d + 4 * idx, v[i].x, v[i].y, v[i].z, v[i].w);
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
            if (out2) ln_store4<float>(out2 + row * d + 4 * idx, y0, y1, y2, y3);
        }
    }
}
