"""The two random-init ``Wav2Vec2ForCTC`` configurations the wav2vec2 tests share (no trained checkpoint ships): A, the base form (GroupNorm behind
the first convolution, no conv bias, post-LN layers), and B, the large / MMS form (LayerNorm behind every convolution, conv bias, pre-LN layers);
both with ``conv_dim = (128,) * 7`` and two layers."""
import functools

FORMS = {
    "A": dict(vocab_size=32, hidden_size=384, num_attention_heads=6, num_conv_pos_embedding_groups=8, feat_extract_norm="group", conv_bias=False,
              do_stable_layer_norm=False),
    "B": dict(vocab_size=40, hidden_size=256, num_attention_heads=4, num_conv_pos_embedding_groups=4, feat_extract_norm="layer", conv_bias=True,
              do_stable_layer_norm=True),
}


def config(form):
    import transformers
    return transformers.Wav2Vec2Config(conv_dim=(128,) * 7, num_hidden_layers=2, intermediate_size=512, num_conv_pos_embeddings=128, **FORMS[form])


@functools.lru_cache(maxsize=None)
def model(form):
    """fp32, eval mode, on the CPU; seeded."""
    import torch
    import transformers
    torch.manual_seed(19 + ord(form))
    return transformers.Wav2Vec2ForCTC(config(form)).eval()
