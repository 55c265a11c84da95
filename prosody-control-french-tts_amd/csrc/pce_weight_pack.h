// pce_weight_pack.h -- the host half of every model loader (Whisper encoder and decoder, BERT, wav2vec2): a weight blob of floats is repacked into
// `mats` (the matrices, converted to the 16-bit operand type on the device) and `vecs` (biases and LayerNorm vectors, which stay fp32); a loader
// keeps each tensor's offset, in elements.  Host only, no HIP: upload_weights (pce_whisper_impl.inc) is the device half, and
// tests/host/weight_pack_main.cpp builds this file alone.
#pragma once
#include <cstddef>
#include <vector>

struct WeightPack {
    std::vector<float> mats, vecs;
    // append n floats and return their offset; mat / vec also advance the blob cursor.  Every vector starts on a multiple of 4 floats (16 bytes)
    size_t mat_at(const float *p, size_t n) { const size_t o = mats.size(); mats.insert(mats.end(), p, p + n); return o; }
    size_t vec_at(const float *p, size_t n) { const size_t o = vecs.size(); vecs.insert(vecs.end(), p, p + n); pad_vecs(); return o; }
    size_t mat(const float *&p, size_t n) { p += n; return mat_at(p - n, n); }
    size_t vec(const float *&p, size_t n) { p += n; return vec_at(p - n, n); }
    size_t zeros(size_t n) { const size_t o = vecs.size(); vecs.insert(vecs.end(), n, 0.f); pad_vecs(); return o; }
    // q.w q.b k.w [k.b] v.w v.b out.w out.b -> the fused projection [3d][d] with its bias [q.b | k.b or zeros | v.b] (one vector: d % 4 == 0),
    // the output projection [d][d] and its bias
    struct Attn { size_t qkv_w, qkv_b, out_w, out_b; };
    Attn self_attention(const float *&p, size_t d, bool key_bias)
    {
        Attn a;
        const float *qw = p, *qb = qw + d * d, *kw = qb + d, *kb = kw + d * d, *vw = key_bias ? kb + d : kb, *vb = vw + d * d;
        a.qkv_w = mat_at(qw, d * d); mat_at(kw, d * d); mat_at(vw, d * d);
        a.qkv_b = vec_at(qb, d);
        if (key_bias) vec_at(kb, d); else zeros(d);
        vec_at(vb, d);
        p = vb + d;
        a.out_w = mat(p, d * d); a.out_b = vec(p, d);
        return a;
    }
    void pad_vecs() { vecs.resize((vecs.size() + 3) & ~(size_t)3); }
};
