// pce_sweep.h -- the REGISTER SWEEP of k_ctc (pce_ctc.hip) and k_wx_trellis (pce_wx.hip): what a thread that owns SWEEP_RUN consecutive states of a
// frame-sequential recurrence exchanges with the outside.  The recurrences themselves stay in their files.  Device only, every function
// force-inlined: both sweeps are marked PCE_NO_PK_F32, and that attribute keeps the runtime's un-attributed helpers (__syncthreads, make_float4)
// out of line -- a call on the serial chain of a latency-bound kernel.  Through the forms below the sweeps hold no call.
//   <false>: a clip whose states fit one wave runs on one wave, no LDS and no barrier, four clips per workgroup.
//   <true>:  one workgroup per clip; the top state of a wave crosses to lane 0 of the next through an LDS slot, double buffered by frame
//            parity: ONE barrier per frame.
// A state's left neighbour is in the thread's own registers, or is the top state of the thread before: ONE DPP wave shift per frame (the idiom of
// k_levenshtein, pce_align.hip).  Emissions depend on the frame only: a sweep loads frame t + 1's while it computes frame t.
#pragma once
#include "pce_wave.h"

constexpr int SWEEP_RUN = 4;                                // states per thread: one trace byte (CTC), one 16-byte row piece (whisperX)
constexpr int SWEEP_MAX_THREADS = 1024;                     // include/pce.h states SWEEP_RUN * SWEEP_MAX_THREADS as both aligners' limit
typedef float SweepXch[2][SWEEP_MAX_THREADS / WAVE_SIZE];   // [frame parity][wave]: the top state of each wave

struct SweepWho { int lane, wave, slot, tid; };             // slot: the place in the launch's id list; tid: the thread's place in its clip
template <bool MULTI> __device__ __forceinline__ SweepWho sweep_who()
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // (slot >= n_ids, <false> only: a whole wave leaves, and that form has no barrier)
    return {lane, wave, MULTI ? (int)blockIdx.x : (int)blockIdx.x * 4 + wave, MULTI ? (int)threadIdx.x : lane};
}
__device__ __forceinline__ void sweep_barrier() { __syncthreads(); }
// s_waitcnt vmcnt(0): the prefetched emissions have landed.  sweep_publish says so between lane 63's LDS store and the barrier (the two latencies
// overlap), sweep_store4 before its store: once per frame, BEFORE the frame's global store, and once before the frame loop.  vmcnt counts loads and
// stores in issue order and the store is conditional, so left alone the compiler waits for the loads after the store -- for the store too, every
// frame -- and loads still pending at the loop's head make it wait at their first use inside, right after the prefetch is issued.  The out-of-line
// runtime helpers waited at these very places by their calling convention; inlined without this, k_wx_trellis and k_ctc<true> ran 20 % longer
// (profiles/r21/sweep_identity.txt).  k_ctc<false> has neither place: the compiler's own waits at the end of the frame body serve it best (same file).
__device__ __forceinline__ void sweep_loads_landed() { __builtin_amdgcn_s_waitcnt(0x0F70); }      // vmcnt 0; expcnt 7 and lgkmcnt 15: not waited for
// wave_shr:1 -- the top state of the thread before; lane 0 takes the wave before's from the slot it published for this parity, the first thread -inf
template <bool MULTI> __device__ __forceinline__ float sweep_left(float top, const SweepXch &xch, int parity, int lane, int wave)
{
    float p = dpp<0x138>(top);
    if (lane == 0) p = (MULTI && wave > 0) ? xch[parity][wave - 1] : -INFINITY;
    return p;
}
template <bool MULTI> __device__ __forceinline__ void sweep_publish(float top, SweepXch &xch, int parity, int lane, int wave)
{
    if (MULTI) {
        if (lane == 63) xch[parity][wave] = top;
        sweep_loads_landed();
        sweep_barrier();
    }
}
// one 16-byte store (p is 16-byte aligned)
__device__ __forceinline__ void sweep_store4(float *p, const float (&a)[SWEEP_RUN])
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    sweep_loads_landed();
    *reinterpret_cast<f4 *>(p) = f4{a[0], a[1], a[2], a[3]};
}
