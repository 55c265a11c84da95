// Stand-alone check of csrc/pce_w2v_seg_plan.h (tests/test_w2v_segments_host.py builds it with ASan + UBSan and runs it): the chunk plan of
// pce_w2v_run_segments on seeded length mixes.  Every segment sits in exactly one chunk, every slot holds its segment, the budget, the row
// limit and segments_per_chunk hold, and the two bounds the header states hold: at most 7 length classes, rows computed <= 2 x (rows valid
// + 15 per segment).  The frame and byte functions are the standard seven-layer stack's and a plain affine cost: the plan takes them as
// arguments.  Exit status 0: every check held.
#include "pce_w2v_seg_plan.h"
#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static const int32_t KERNEL[7] = {10, 3, 3, 3, 3, 2, 2}, STRIDE[7] = {5, 2, 2, 2, 2, 2, 2};

static int64_t frames_of(int64_t samples)
{
    int64_t t[7];
    w2v_seg_layer_frames(KERNEL, STRIDE, 7, samples, t);
    return t[6];
}
static int64_t slot_bytes(int64_t samples) { return 4096 * w2v_seg_rows_pad(frames_of(samples)) + 6 * samples; }
// the first sample count that gives `frames` frames
static int64_t samples_of(int64_t frames) { return 400 + 320 * (frames - 1); }

struct Case { const char *name; std::vector<int64_t> samples; int per_chunk; int64_t budget, row_limit; };

static void check(const Case &cs)
{
    const std::vector<int64_t> &s = cs.samples;
    const W2vSegPlan p = w2v_seg_plan(s, cs.per_chunk, cs.budget, cs.row_limit, frames_of, slot_bytes);
    const size_t n = s.size();
    CHECK(p.order.size() == n);
    std::vector<int> seen(n, 0);
    for (int j : p.order) { CHECK(j >= 0 && (size_t)j < n); if (j >= 0 && (size_t)j < n) seen[(size_t)j]++; }
    for (size_t j = 0; j < n; j++) CHECK(seen[j] == 1);                               // every segment once
    for (size_t i = 1; i < n; i++) {                                                  // longest first, equal lengths in the caller's order
        const int a = p.order[i - 1], b = p.order[i];
        CHECK(s[(size_t)a] > s[(size_t)b] || (s[(size_t)a] == s[(size_t)b] && a < b));
    }
    size_t next = 0;
    int64_t computed = 0, valid = 0;
    int classes = p.chunks.empty() ? 0 : 1;
    for (size_t k = 0; k < p.chunks.size(); k++) {
        const W2vSegChunk &ch = p.chunks[k];
        CHECK(ch.first == next && ch.count >= 1 && ch.first + ch.count <= n);         // the chunks tile the order: each segment in exactly one
        if (ch.first != next || ch.first + ch.count > n) return;
        next = ch.first + ch.count;
        CHECK(ch.samples == s[(size_t)p.order[ch.first]] && ch.T == frames_of(ch.samples) && ch.T_pad == w2v_seg_rows_pad(ch.T) && ch.T_pad % 16 == 0);
        int64_t lt[7];
        w2v_seg_layer_frames(KERNEL, STRIDE, 7, ch.samples, lt);
        for (size_t i = 0; i < ch.count; i++) {
            const int64_t sj = s[(size_t)p.order[ch.first + i]], Tj = frames_of(sj);
            int64_t t[7];
            w2v_seg_layer_frames(KERNEL, STRIDE, 7, sj, t);
            for (int l = 0; l < 7; l++) CHECK(t[l] <= lt[l]);                         // the slot holds the segment at every layer
            CHECK(Tj >= 1 && Tj <= ch.T && 2 * w2v_seg_rows_pad(Tj) >= ch.T_pad);
            valid += Tj;
        }
        computed += (int64_t)ch.count * ch.T_pad;
        if (ch.count > 1) {                                                           // (a chunk holds its opener whatever the limits say)
            CHECK((int64_t)ch.count * slot_bytes(ch.samples) <= cs.budget);
            CHECK((int64_t)ch.count * ch.T_pad <= cs.row_limit);
        }
        CHECK(ch.count <= (size_t)W2V_SEG_CHUNK_MAX && (cs.per_chunk <= 0 || ch.count <= (size_t)cs.per_chunk));
        CHECK((int64_t)ch.count * ch.T_pad <= INT32_MAX);
        if (k && 2 * ch.T_pad < p.chunks[k - 1].T_pad) classes++;                     // the length rule closed the chunk before
    }
    CHECK(next == n);
    CHECK(computed == p.rows_computed && valid == p.rows_valid);
    CHECK(classes <= 7);
    CHECK(p.rows_computed <= 2 * (p.rows_valid + 15 * (int64_t)n));
    std::printf("%-28s %5zu segments %4zu chunks %d classes  rows %lld / %lld\n", cs.name, n, p.chunks.size(), classes, (long long)p.rows_computed,
                (long long)p.rows_valid);
}

int main()
{
    CHECK(frames_of(399) == 0 && frames_of(400) == 1 && frames_of(719) == 1 && frames_of(720) == 2 && frames_of(479999) == 1499 && frames_of(480000) == 1499);
    CHECK(w2v_seg_rows_pad(1) == 16 && w2v_seg_rows_pad(16) == 16 && w2v_seg_rows_pad(17) == 32 && w2v_seg_rows_pad(0) == 0);
    const int64_t big = (int64_t)3 << 30, rows = ((int64_t)1 << 31) / 4096;
    std::mt19937_64 rng(21);
    std::vector<int64_t> equal(300, 80000), different, lonely(301, 400), uniform, nothing;
    for (int f = 1; f <= 1500; f += 7) different.push_back(samples_of(f) + (f % 320));
    std::shuffle(different.begin(), different.end(), rng);
    lonely[137] = samples_of(1500);
    for (int i = 0; i < 256; i++) uniform.push_back(8000 + (int64_t)(rng() % 184000));   // 0.5 .. 12 s
    const Case cases[] = {
        {"all equal", equal, 0, big, rows},
        {"all equal, 7 per chunk", equal, 7, big, rows},
        {"all equal, tight budget", equal, 0, 10 * slot_bytes(80000) + 1, rows},
        {"all equal, tight rows", equal, 0, big, 5 * 256 - 1},
        {"all different", different, 0, big, rows},
        {"all different, tight budget", different, 0, 3 * slot_bytes(samples_of(1500)), rows},
        {"one long among 300 short", lonely, 0, big, rows},
        {"one per chunk", different, 1, big, rows},
        {"uniform 0.5-12 s", uniform, 0, big, rows},
        {"budget below one slot", equal, 0, 1, 1},
        {"no segments", nothing, 0, big, rows},
    };
    for (const Case &cs : cases) check(cs);
    {   // all equal: one chunk; tight budget: chunks of 10; one per chunk: as many chunks as segments; the lonely mix: two chunks
        CHECK(w2v_seg_plan(equal, 0, big, rows, frames_of, slot_bytes).chunks.size() == 1);
        CHECK(w2v_seg_plan(equal, 0, 10 * slot_bytes(80000) + 1, rows, frames_of, slot_bytes).chunks.size() == 30);
        CHECK(w2v_seg_plan(different, 1, big, rows, frames_of, slot_bytes).chunks.size() == different.size());
        const W2vSegPlan p = w2v_seg_plan(lonely, 0, big, rows, frames_of, slot_bytes);
        CHECK(p.chunks.size() == 2 && p.chunks[0].count == 1 && p.order[0] == 137 && p.chunks[1].count == 300 && p.chunks[1].T_pad == 16);
        CHECK(w2v_seg_plan(equal, 0, 1, 1, frames_of, slot_bytes).chunks.size() == equal.size());
    }
    return failures ? 1 : 0;
}
