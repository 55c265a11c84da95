// pce_sweep_plan.h -- the launch plan of the two register-sweep aligners (pce_ctc_align, pce_wx_align): the clip record, the thread-count class of a
// clip, the groups of consecutive clips whose storage fits a budget, the id lists and launches per group.  Host only, no HIP, pure functions
// over vectors: tests/host/sweep_plan_main.cpp builds this file alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct SweepClip {
    long long row0;      // first emission row
    long long seq0;      // first target / token (and first tok_first / tok_last entry)
    long long st0;       // first word of its trace / trellis table inside the group's buffer
    long long out0;      // first entry of the per-frame outputs (whisperX: and of wmax, and x 8 of the back-track record)
    long long scr0;      // CTC's general form: first float of its two alpha rows
    int T, n;            // frames; targets L / tokens J
    int stride;          // words per row of st0's storage: CTC: threads (register form) or groups of 4 states (general form) per frame of trace; whisperX: J rounded up to 4
    int wild;            // whisperX: the clip holds a wildcard (wmax is valid for its frames)
};

// 0: one wave (<= 64 threads); 1..4: 128 / 256 / 512 / 1024 threads
inline int sweep_kind(int64_t threads)
{
    int k = 0;
    for (int64_t nt = 64; nt < threads; nt <<= 1) k++;
    return k;
}

// Groups of consecutive clips whose storage fits the budget together.  words[q] < 0: clip q is not run (it takes no room and opens no group).
struct SweepGroups {
    std::vector<int64_t> offset;        // per clip: its first word inside its group's buffer (0 for a clip that is not run)
    std::vector<size_t> group_end;      // one past the last clip of every group; always ends with n
    int64_t largest = 0;                // words of the largest group
    ptrdiff_t too_large = -1;           // the first clip that alone exceeds the budget (the plan stops there), else -1
};
inline SweepGroups sweep_groups(const std::vector<int64_t> &words, int64_t budget)
{
    SweepGroups g;
    g.offset.assign(words.size(), 0);
    int64_t used = 0;
    for (size_t q = 0; q < words.size(); q++) {
        const int64_t w = words[q];
        if (w < 0) continue;
        if (w > budget) { g.too_large = (ptrdiff_t)q; return g; }
        if (used + w > budget) { g.group_end.push_back(q); used = 0; }
        g.offset[q] = used;
        used += w;
        g.largest = std::max(g.largest, used);
    }
    g.group_end.push_back(words.size());
    return g;
}

// Per group: one launch per sweep kind 0 .. n_kinds - 1 in use (ascending; kind[q] < 0: not run), then one of tail_kind over the group's whole id
// range.  ids[first .. first + count) are the launch's clips; the lists are appended to what ids holds.  g0 .. ge: the group's clips.
struct SweepLaunch { int kind; size_t first, count, g0, ge; };
inline std::vector<SweepLaunch> sweep_launches(const std::vector<int> &kind, const std::vector<size_t> &group_end, int n_kinds, int tail_kind, std::vector<int> &ids)
{
    std::vector<SweepLaunch> launches;
    size_t g0 = 0;
    for (size_t ge : group_end) {
        const size_t first_of_group = ids.size();
        for (int k = 0; k < n_kinds; k++) {
            const size_t first = ids.size();
            for (size_t q = g0; q < ge; q++) if (kind[q] == k) ids.push_back((int)q);
            if (ids.size() > first) launches.push_back({k, first, ids.size() - first, g0, ge});
        }
        if (ids.size() > first_of_group) launches.push_back({tail_kind, first_of_group, ids.size() - first_of_group, g0, ge});
        g0 = ge;
    }
    return launches;
}
