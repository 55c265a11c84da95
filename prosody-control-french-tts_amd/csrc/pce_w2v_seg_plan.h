// pce_w2v_seg_plan.h -- the chunk plan of pce_w2v_run_segments: frames of a segment at every layer of the feature encoder, and the chunks of
// segments of similar length that run through one set of launches.  Host only, no HIP, pure functions over vectors:
// tests/host/w2v_seg_plan_main.cpp builds this file alone.
//
// A chunk's launches cover count slots of the rows of its first (longest) segment, so a chunk costs count x slot rows whatever its members hold.
// The rule: segments in descending order of their sample count (stable; the frame count at every layer is monotone in it, so the first
// segment of a chunk has the most rows at EVERY layer, not only behind the last); a chunk opens with the longest segment left and takes the
// following ones while the caller's segments_per_chunk, the image budget and the launchers' int row counts allow it and the segment's padded
// frame count is at least half the slot's.  That bounds the waste: rows computed <= 2 x (rows valid + 15 per segment), and since an opener's
// slot is less than half of the one before whenever the length rule closed a chunk, slots of 16 .. 1504 rows give at most 6 such steps.
// The plan decides speed only: no kernel reduces across segments and none is chosen by the row count.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

constexpr int W2V_SEG_ROW_PAD = 16;            // frames of a slot behind the last convolution: a multiple of this
constexpr int W2V_SEG_CHUNK_MAX = 4096;        // segments of one chunk, at most (grid dimensions, table sizes)

// frames of `samples` input samples behind each of n_conv convolutions (no padding: floor((L - k) / s) + 1, 0 once L < k)
inline void w2v_seg_layer_frames(const int32_t *kernel, const int32_t *stride, int n_conv, int64_t samples, int64_t *frames)
{
    int64_t t = samples;
    for (int i = 0; i < n_conv; i++) { t = t >= kernel[i] ? (t - kernel[i]) / stride[i] + 1 : 0; frames[i] = t; }
}
inline int64_t w2v_seg_rows_pad(int64_t T) { return (T + W2V_SEG_ROW_PAD - 1) / W2V_SEG_ROW_PAD * W2V_SEG_ROW_PAD; }

struct W2vSegChunk { size_t first, count; int64_t samples, T, T_pad; };      // order[first .. first + count); the opener's samples, frames, slot rows
struct W2vSegPlan {
    std::vector<int> order;                  // segment indices, longest first
    std::vector<W2vSegChunk> chunks;
    int64_t rows_computed = 0, rows_valid = 0;
};

// samples[j]: the samples segment j is run on (its own, or min_samples).  frames_of(samples) -> frames behind the last convolution;
// slot_bytes(samples) -> bytes of one slot's activation images in a chunk that such a segment opens.  per_chunk: 0 = by budget.
// row_limit: slots x slot rows of one chunk, at most.  A chunk holds its opener whatever the limits say.
template <class Frames, class SlotBytes>
inline W2vSegPlan w2v_seg_plan(const std::vector<int64_t> &samples, int per_chunk, int64_t budget, int64_t row_limit, Frames frames_of, SlotBytes slot_bytes)
{
    W2vSegPlan p;
    const size_t n = samples.size();
    p.order.resize(n);
    std::iota(p.order.begin(), p.order.end(), 0);
    std::stable_sort(p.order.begin(), p.order.end(), [&](int a, int b) { return samples[(size_t)a] > samples[(size_t)b]; });
    size_t i = 0;
    while (i < n) {
        W2vSegChunk ch{i, 1, samples[(size_t)p.order[i]], 0, 0};
        ch.T = frames_of(ch.samples); ch.T_pad = w2v_seg_rows_pad(ch.T);
        const int64_t bytes = std::max<int64_t>(1, slot_bytes(ch.samples));
        int64_t cap = std::min<int64_t>(W2V_SEG_CHUNK_MAX, std::max<int64_t>(1, budget / bytes));
        if (per_chunk > 0) cap = std::min<int64_t>(cap, per_chunk);
        if (ch.T_pad > 0) cap = std::min<int64_t>(cap, std::max<int64_t>(1, row_limit / ch.T_pad));
        p.rows_valid += ch.T;
        for (size_t j = i + 1; j < n && (int64_t)ch.count < cap; j++) {
            const int64_t T = frames_of(samples[(size_t)p.order[j]]);
            if (2 * w2v_seg_rows_pad(T) < ch.T_pad) break;
            p.rows_valid += T;
            ch.count++;
        }
        p.rows_computed += (int64_t)ch.count * ch.T_pad;
        p.chunks.push_back(ch);
        i += ch.count;
    }
    return p;
}
