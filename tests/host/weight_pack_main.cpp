// Stand-alone check of csrc/pce_weight_pack.h (tests/test_weight_pack_host.py builds it with ASan + UBSan and runs it): the blob is
// float(index) in a heap allocation of exactly the expected size, so every packed value names the blob position it must have come from and a
// read past the blob is caught.  Exit status 0: every check held.
#include "pce_weight_pack.h"
#include <cstdio>
#include <memory>

static int failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

// all n values from `at` on are first, first + 1, ...
static bool iota_at(const std::vector<float> &v, size_t at, size_t n, size_t first)
{
    if (at + n > v.size()) return false;
    for (size_t i = 0; i < n; i++)
        if (v[at + i] != (float)(first + i)) return false;
    return true;
}
static bool zeros_at(const std::vector<float> &v, size_t at, size_t n)
{
    if (at + n > v.size()) return false;
    for (size_t i = 0; i < n; i++)
        if (v[at + i] != 0.f) return false;
    return true;
}

static void self_attention(bool key_bias)
{
    const size_t d = 128, dd = d * d, n = 4 * dd + (key_bias ? 4 : 3) * d;       // (every index is below 2^24: exact in a float)
    std::unique_ptr<float[]> blob(new float[n]);
    for (size_t i = 0; i < n; i++) blob[i] = (float)i;
    WeightPack pk;
    float lead[8] = {-1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f, -1.f};            // something in front, so that the offsets are not zero
    pk.mat_at(lead, 8); pk.vec_at(lead, 8);
    const float *p = blob.get();
    const WeightPack::Attn a = pk.self_attention(p, d, key_bias);
    CHECK(p == blob.get() + n);
    // blob order: q.w q.b k.w [k.b] v.w v.b out.w out.b
    const size_t qw = 0, qb = dd, kw = qb + d, kb = kw + dd, vw = key_bias ? kb + d : kb, vb = vw + dd, ow = vb + d, ob = ow + dd;
    CHECK(a.qkv_w == 8 && a.out_w == 8 + 3 * dd && pk.mats.size() == 8 + 4 * dd);
    CHECK(iota_at(pk.mats, a.qkv_w, dd, qw) && iota_at(pk.mats, a.qkv_w + dd, dd, kw) && iota_at(pk.mats, a.qkv_w + 2 * dd, dd, vw));
    CHECK(iota_at(pk.mats, a.out_w, dd, ow));
    CHECK(a.qkv_b == 8 && a.out_b == 8 + 3 * d && pk.vecs.size() == 8 + 4 * d);
    CHECK(iota_at(pk.vecs, a.qkv_b, d, qb));
    CHECK(key_bias ? iota_at(pk.vecs, a.qkv_b + d, d, kb) : zeros_at(pk.vecs, a.qkv_b + d, d));
    CHECK(iota_at(pk.vecs, a.qkv_b + 2 * d, d, vb));
    CHECK(iota_at(pk.vecs, a.out_b, d, ob));
    for (size_t i = 0; i < 8; i++) CHECK(pk.mats[i] == -1.f && pk.vecs[i] == -1.f);         // what was there stays
}

static void vector_alignment()
{
    std::unique_ptr<float[]> blob(new float[11]);
    for (size_t i = 0; i < 11; i++) blob[i] = (float)(i + 1);                    // non-zero, so that the padding shows
    WeightPack pk;
    const float *p = blob.get();
    const size_t a = pk.vec(p, 1), b = pk.vec(p, 4), c = pk.vec(p, 6), z = pk.zeros(3), e = pk.vec_at(blob.get(), 2);
    CHECK(p == blob.get() + 11);
    CHECK(a == 0 && b == 4 && c == 8 && z == 16 && e == 20 && pk.vecs.size() == 24);
    CHECK(iota_at(pk.vecs, a, 1, 1) && zeros_at(pk.vecs, 1, 3));
    CHECK(iota_at(pk.vecs, b, 4, 2));
    CHECK(iota_at(pk.vecs, c, 6, 6) && zeros_at(pk.vecs, 14, 2));
    CHECK(zeros_at(pk.vecs, z, 4));
    CHECK(iota_at(pk.vecs, e, 2, 1) && zeros_at(pk.vecs, 22, 2));
    // matrices are packed back to back, and the forms that take the cursor advance it by what they copied
    p = blob.get();
    const size_t m0 = pk.mat(p, 3), m1 = pk.mat_at(p, 5);
    CHECK(m0 == 0 && m1 == 3 && p == blob.get() + 3 && pk.mats.size() == 8 && iota_at(pk.mats, 0, 8, 1));
}

int main()
{
    self_attention(false);
    self_attention(true);
    vector_alignment();
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
