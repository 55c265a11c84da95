// Stand-alone check of csrc/pce_sweep_plan.h (tests/test_sweep_plan_host.py builds it with ASan + UBSan and runs it): the thread-count classes, the
// groups of clips under a budget and the launch lists of pce_ctc_align / pce_wx_align.  Every input vector has exactly the size the plan may
// read, so an index one past it is caught.  Exit status 0: every check held.
#include "pce_sweep_plan.h"
#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

using I64 = std::vector<int64_t>;
using Ends = std::vector<size_t>;
using Ints = std::vector<int>;

static void kinds()
{
    CHECK(sweep_kind(1) == 0 && sweep_kind(64) == 0);
    CHECK(sweep_kind(65) == 1 && sweep_kind(128) == 1);
    CHECK(sweep_kind(129) == 2);
    CHECK(sweep_kind(512) == 3);
    CHECK(sweep_kind(513) == 4 && sweep_kind(1024) == 4);
}

static void groups()
{
    {   // an exact fit: one group
        const SweepGroups g = sweep_groups(I64{4, 3, 3}, 10);
        CHECK(g.too_large == -1 && g.group_end == Ends{3} && g.offset == (I64{0, 4, 7}) && g.largest == 10);
    }
    {   // one word over: a new group opens at that clip
        const SweepGroups g = sweep_groups(I64{4, 3, 4, 1}, 10);
        CHECK(g.too_large == -1 && g.group_end == (Ends{2, 4}) && g.offset == (I64{0, 4, 0, 4}) && g.largest == 7);
    }
    {   // clips that are not run, at the start, in the middle and at the end of a group: no room, no group
        const SweepGroups g = sweep_groups(I64{-1, 6, -1, 4, -1, -1, 5, -1}, 10);
        CHECK(g.too_large == -1 && g.group_end == (Ends{6, 8}) && g.offset == (I64{0, 0, 0, 6, 0, 0, 0, 0}) && g.largest == 10);
    }
    {   // a clip of 0 words is run and takes no room
        const SweepGroups g = sweep_groups(I64{10, 0, 1}, 10);
        CHECK(g.too_large == -1 && g.group_end == (Ends{2, 3}) && g.offset == (I64{0, 10, 0}) && g.largest == 10);
    }
    {   // a single clip over the budget: its index, whatever stands before it
        CHECK(sweep_groups(I64{11}, 10).too_large == 0);
        CHECK(sweep_groups(I64{-1, 10, 3, 11, 2}, 10).too_large == 3);
        CHECK(sweep_groups(I64{10}, 10).too_large == -1);
    }
    {   // nothing runs: one group, and no launch from it
        const SweepGroups g = sweep_groups(I64{-1, -1, -1}, 10);
        CHECK(g.too_large == -1 && g.group_end == Ends{3} && g.offset == (I64{0, 0, 0}) && g.largest == 0);
        Ints ids;
        CHECK(sweep_launches(Ints{-1, -1, -1}, g.group_end, 5, 5, ids).empty() && ids.empty());
    }
}

static bool is(const SweepLaunch &l, int kind, size_t first, size_t count, size_t g0, size_t ge)
{
    return l.kind == kind && l.first == first && l.count == count && l.g0 == g0 && l.ge == ge;
}

static void launches()
{
    // three groups: clips 0 .. 4 (kinds 2, 0, -1, 2, 5), clips 5 .. 6 (none runs), clips 7 .. 9 (kinds 1, -1, 0); ids keeps what it held
    const Ints kind{2, 0, -1, 2, 5, -1, -1, 1, -1, 0};
    Ints ids{42};
    const std::vector<SweepLaunch> l = sweep_launches(kind, Ends{5, 7, 10}, 6, 6, ids);
    CHECK(ids == (Ints{42, 1, 0, 3, 4, 9, 7}));
    CHECK(l.size() == 7);
    if (l.size() == 7) {
        CHECK(is(l[0], 0, 1, 1, 0, 5) && is(l[1], 2, 2, 2, 0, 5) && is(l[2], 5, 4, 1, 0, 5));
        CHECK(is(l[3], 6, 1, 4, 0, 5));                      // the tail: the group's whole id range
        CHECK(is(l[4], 0, 5, 1, 7, 10) && is(l[5], 1, 6, 1, 7, 10) && is(l[6], 6, 5, 2, 7, 10));
    }
    // whisperX's shape (five sweep kinds, tail 5), a fresh id list, kinds descending in clip order
    Ints ids2;
    const std::vector<SweepLaunch> m = sweep_launches(Ints{4, 0}, Ends{2}, 5, 5, ids2);
    CHECK(ids2 == (Ints{1, 0}) && m.size() == 3);
    if (m.size() == 3) CHECK(is(m[0], 0, 0, 1, 0, 2) && is(m[1], 4, 1, 1, 0, 2) && is(m[2], 5, 0, 2, 0, 2));
}

int main()
{
    kinds();
    groups();
    launches();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
