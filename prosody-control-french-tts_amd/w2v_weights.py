"""Weights of a ``transformers`` ``Wav2Vec2ForCTC`` model (wav2vec2 / MMS) for ``pce_w2v_load``: dims from a config, tensor names and blob
shapes in the order of the flat float32 blob, and a packer for a ``state_dict``.

What the packer changes on the way: convolution weights ``[out][in][tap]`` become ``[out][tap][in]`` (the feature encoder's layers 1-6 and the
positional convolution run as GEMMs over time-major images, K = (tap, channel)); the positional convolution's weight norm (over dimensions 0
and 1, one gain per tap: ``weight_norm(conv, dim=2)``) is folded into plain weights, from either spelling of its parameters; ``masked_spec_embed``
is dropped; the ``wav2vec2.`` prefix of ``Wav2Vec2ForCTC`` is accepted and optional."""
from __future__ import annotations

import numpy as np

POS_G = ("pos_conv_embed.conv.parametrizations.weight.original0", "pos_conv_embed.conv.weight_g")
POS_V = ("pos_conv_embed.conv.parametrizations.weight.original1", "pos_conv_embed.conv.weight_v")
POS_W = "encoder.pos_conv_embed.conv.weight"          # the folded weight's name in tensor_order


def dims(config) -> dict:
    """``transformers.Wav2Vec2Config`` -> dims of ``pce_w2v_dims`` (exact GELU, no adapter, a CTC head on the hidden size)."""
    if config.feat_extract_norm not in ("group", "layer"):
        raise ValueError(f"feat_extract_norm {config.feat_extract_norm!r}: 'group' or 'layer'")
    if config.feat_extract_activation != "gelu" or config.hidden_act != "gelu":
        raise ValueError("the kernels hold the exact GELU in the feature encoder and in the feed-forward")
    if getattr(config, "add_adapter", False):
        raise ValueError("adapters are not supported")
    if getattr(config, "position_embeddings_type", "convolutional") not in (None, "convolutional"):
        raise ValueError("convolutional positional embeddings only")
    return dict(n_conv=len(config.conv_dim), conv_dim=tuple(int(x) for x in config.conv_dim), conv_kernel=tuple(int(x) for x in config.conv_kernel),
                conv_stride=tuple(int(x) for x in config.conv_stride), feat_norm=0 if config.feat_extract_norm == "group" else 1,
                conv_bias=int(bool(config.conv_bias)), n_state=int(config.hidden_size), n_head=int(config.num_attention_heads),
                n_inter=int(config.intermediate_size), n_layer=int(config.num_hidden_layers), stable_ln=int(bool(config.do_stable_layer_norm)),
                pos_taps=int(config.num_conv_pos_embeddings), pos_groups=int(config.num_conv_pos_embedding_groups), n_vocab=int(config.vocab_size),
                ln_eps=float(config.layer_norm_eps))


def tensor_order(dims):
    """[(name without the ``wav2vec2.`` prefix, shape IN THE BLOB)] -- convolution weights already as [out][tap][in]."""
    d, inter, layer_norm = dims["n_state"], dims["n_inter"], dims["feat_norm"] == 1
    order = []
    for i in range(dims["n_conv"]):
        p = f"feature_extractor.conv_layers.{i}."
        c_in, c_out = (dims["conv_dim"][i - 1] if i else 1), dims["conv_dim"][i]
        order.append((p + "conv.weight", (c_out, dims["conv_kernel"][i], c_in)))
        if dims["conv_bias"]:
            order.append((p + "conv.bias", (c_out,)))
        if layer_norm or i == 0:
            order += [(p + "layer_norm.weight", (c_out,)), (p + "layer_norm.bias", (c_out,))]
    c6 = dims["conv_dim"][-1]
    order += [("feature_projection.layer_norm.weight", (c6,)), ("feature_projection.layer_norm.bias", (c6,)),
              ("feature_projection.projection.weight", (d, c6)), ("feature_projection.projection.bias", (d,)),
              (POS_W, (d, dims["pos_taps"], d // dims["pos_groups"])), ("encoder.pos_conv_embed.conv.bias", (d,)),
              ("encoder.layer_norm.weight", (d,)), ("encoder.layer_norm.bias", (d,))]
    for l in range(dims["n_layer"]):
        p = f"encoder.layers.{l}."
        order += [(p + "attention.q_proj.weight", (d, d)), (p + "attention.q_proj.bias", (d,)),
                  (p + "attention.k_proj.weight", (d, d)), (p + "attention.k_proj.bias", (d,)),
                  (p + "attention.v_proj.weight", (d, d)), (p + "attention.v_proj.bias", (d,)),
                  (p + "attention.out_proj.weight", (d, d)), (p + "attention.out_proj.bias", (d,)),
                  (p + "layer_norm.weight", (d,)), (p + "layer_norm.bias", (d,)),
                  (p + "feed_forward.intermediate_dense.weight", (inter, d)), (p + "feed_forward.intermediate_dense.bias", (inter,)),
                  (p + "feed_forward.output_dense.weight", (d, inter)), (p + "feed_forward.output_dense.bias", (d,)),
                  (p + "final_layer_norm.weight", (d,)), (p + "final_layer_norm.bias", (d,))]
    return order + [("lm_head.weight", (dims["n_vocab"], d)), ("lm_head.bias", (dims["n_vocab"],))]


def n_floats(dims) -> int:
    return int(sum(int(np.prod(shape)) for _, shape in tensor_order(dims)))


def _np(a):
    return np.asarray(a.detach().cpu().float().numpy() if hasattr(a, "detach") else a, dtype=np.float32)


def fold_pos_conv(W) -> np.ndarray:
    """The positional convolution's plain weight ``[out][in / groups][tap]`` = g v / ||v||, the norm over dimensions 0 and 1 per tap, from a
    ``state_dict`` without the ``wav2vec2.`` prefix (either spelling of the weight norm, or an already plain ``conv.weight``)."""
    for gk, vk in zip(POS_G, POS_V):
        if "encoder." + gk in W:
            g, v = _np(W["encoder." + gk]).astype(np.float64), _np(W["encoder." + vk]).astype(np.float64)
            norm = np.sqrt((v * v).sum(axis=(0, 1), keepdims=True))
            return (v * (g / norm)).astype(np.float32)
    return _np(W[POS_W])


def unfold_pos_conv(blob_weight) -> np.ndarray:
    """The blob's ``[out][tap][in / groups]`` back as ``conv.weight``'s ``[out][in / groups][tap]``."""
    return np.ascontiguousarray(np.transpose(np.asarray(blob_weight), (0, 2, 1)))


def pack(state_dict, dims) -> np.ndarray:
    """``state_dict`` of a ``Wav2Vec2ForCTC`` (or of its ``wav2vec2`` body plus ``lm_head``) -> the flat float32 blob of ``tensor_order``."""
    W = {(k[len("wav2vec2."):] if k.startswith("wav2vec2.") else k): v for k, v in state_dict.items()}
    W.pop("masked_spec_embed", None)
    out = []
    for name, shape in tensor_order(dims):
        if name == POS_W:
            a = np.transpose(fold_pos_conv(W), (0, 2, 1))
        elif name.endswith("conv.weight"):
            a = np.transpose(_np(W[name]), (0, 2, 1))
        else:
            a = _np(W[name])
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(a.shape)}, expected {tuple(shape)}")
        out.append(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
    return np.concatenate(out)
