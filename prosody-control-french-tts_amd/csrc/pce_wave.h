// pce_wave.h -- the wave-level reductions and lane moves of every kernel file (device only, force-inlined: a kernel marked PCE_NO_PK_F32
// keeps its attribute through them).  The order of a floating-point reduction decides its bits and the tests compare bits, so:
// ONE TREE PER NAME.  Two functions that differ in tree (xor / down, butterfly / DPP row, association of the four row totals) have two
// names; no kernel is moved from one to another without its own measurement, and a new kernel file adds no copy of its own.
#pragma once
#include <hip/hip_runtime.h>

constexpr int WAVE_SIZE = 64;
#if defined(__HIP_DEVICE_COMPILE__)
// (the compiler offers no constant for the target's wavefront size; the GFX9 family -- GCN, CDNA, gfx950 -- executes 64-lane wavefronts only)
#if defined(__GFX9__)
static_assert(WAVE_SIZE == 64, "every helper below is written for 64-lane wavefronts");
#else
#error "pce_wave.h: a target with 64-lane wavefronts (GFX9 family) is required"
#endif
#endif

__device__ __forceinline__ int wave_max2(int a, int b) { return max(a, b); }
__device__ __forceinline__ float wave_max2(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double wave_max2(double a, double b) { return fmax(a, b); }

// ---- butterflies by __shfl_xor (ds_bpermute): offsets W/2, W/4, .. 1; every lane of an aligned group of W lanes holds the group's result,
// the same bits in each (step k combines v[lane] with v[lane ^ off]: both partners form the same sum)
template <int W = WAVE_SIZE, class T> __device__ __forceinline__ T wave_xor_sum(T v)
{
    for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE_SIZE);
    return v;
}
template <int W = WAVE_SIZE, class T> __device__ __forceinline__ T wave_xor_max(T v)
{
    for (int off = W / 2; off > 0; off >>= 1) v = wave_max2(v, __shfl_xor(v, off, WAVE_SIZE));
    return v;
}

// ---- reduction by __shfl_down: offsets 32, 16, .. 1, v[lane] += v[lane + off]; LANE 0 ONLY holds the wave's sum
template <class T> __device__ __forceinline__ T wave_down_sum(T v)
{
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE_SIZE);
    return v;
}

// ---- DPP moves (no LDS, no ds_bpermute): lane i receives v of the lane CTRL names; a lane without a source receives 0
template <int CTRL> __device__ __forceinline__ int dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
template <int CTRL> __device__ __forceinline__ float dpp(float v) { return __builtin_bit_cast(float, dpp<CTRL>(__builtin_bit_cast(int, v))); }
template <int CTRL> __device__ __forceinline__ double dpp(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = dpp<CTRL>(lo);
    hi = dpp<CTRL>(hi);
    return __hiloint2double(hi, lo);
}
// Balanced tree inside a 16-lane DPP row: lane pairs, quads, half rows (N >= 8), rows (N == 16); every lane of an aligned group of N lanes
// holds the group's result, the same bits in each.
template <int N, class T> __device__ __forceinline__ T dpp_row_sum(T v)
{
    static_assert(N == 4 || N == 8 || N == 16, "groups of 4, 8 or 16 lanes");
    v += dpp<0xB1>(v);                      // quad_perm [1,0,3,2]
    v += dpp<0x4E>(v);                      // quad_perm [2,3,0,1]
    if (N >= 8) v += dpp<0x141>(v);         // row_half_mirror
    if (N == 16) v += dpp<0x140>(v);        // row_mirror
    return v;
}
template <int N, class T> __device__ __forceinline__ T dpp_row_max(T v)
{
    static_assert(N == 4 || N == 8 || N == 16, "groups of 4, 8 or 16 lanes");
    v = wave_max2(v, dpp<0xB1>(v));
    v = wave_max2(v, dpp<0x4E>(v));
    if (N >= 8) v = wave_max2(v, dpp<0x141>(v));
    if (N == 16) v = wave_max2(v, dpp<0x140>(v));
    return v;
}
// Wave totals: the row tree, then four v_readlane combine the rows on the scalar unit; the result is wave-uniform.
__device__ __forceinline__ int wave_dpp_sum_i32(int v)          // ((r0 + r1) + r2) + r3
{
    v = dpp_row_sum<16>(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ int wave_dpp_max_i32(int v)          // max(max(r0, r1), max(r2, r3))
{
    v = dpp_row_max<16>(v);
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ float wave_dpp_sum_f32(float v)      // (r0 + r1) + (r2 + r3)
{
    const int b = __builtin_bit_cast(int, dpp_row_sum<16>(v));
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
    return (r0 + r1) + (r2 + r3);
}

// ---- 64-bit lane moves from two 32-bit halves
__device__ __forceinline__ double readlane_f64(double v, int src)       // src wave-uniform (v_readlane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_f64(double v, int src)           // src per lane
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl(lo, src, WAVE_SIZE); hi = __shfl(hi, src, WAVE_SIZE);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shfl_up_f64(double v, int d)          // from lane - d; lanes below d keep their own value
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_up(lo, d, WAVE_SIZE); hi = __shfl_up(hi, d, WAVE_SIZE);
    return __hiloint2double(hi, lo);
}
