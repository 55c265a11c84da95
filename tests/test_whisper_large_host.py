"""Whisper large-v3 and large-v3-turbo on the host side: the model table rows (the names openai-whisper 20240930 resolves, "large" and
"turbo" among them), their built-in alignment heads, and a turbo-shaped miniature checkpoint (d = 1280, 20 heads, 128 mels, 4 decoder
layers, one more language token) loading with the v3 vocabulary."""
import base64

import numpy as np

from prosody_control_french_tts_amd import whisper_weights as WW
from prosody_control_french_tts_amd.Aligners import checkpoint as CK
from prosody_control_french_tts_amd.Aligners.tokenizer import WhisperTokenizer

ENC = dict(n_mels=128, n_ctx=1500, n_state=1280, n_head=20, n_layer=32)


def test_model_table_rows_of_large_v3_and_turbo():
    for name in ("large-v3", "large", "large-v3-turbo", "turbo"):
        assert WW.DIMS[name] == ENC, name
    assert WW.TEXT_DIMS["large-v3"] == WW.TEXT_DIMS["large"] == dict(n_vocab=51866, n_text_ctx=448, n_state=1280, n_head=20, n_layer=32)
    assert WW.TEXT_DIMS["large-v3-turbo"] == WW.TEXT_DIMS["turbo"] == dict(n_vocab=51866, n_text_ctx=448, n_state=1280, n_head=20, n_layer=4)
    # the encoder blob of the full model packs to the published parameter count of large-v3's encoder (635 M without the fixed sinusoids)
    assert sum(int(np.prod(s)) for _, s in WW.tensor_order(WW.DIMS["turbo"])) == 635_048_960


def test_builtin_alignment_heads_of_large_v3_and_turbo():
    assert CK.builtin_alignment_heads("turbo", 4, 20) == [[2, 4], [2, 11], [3, 3], [3, 6], [3, 11], [3, 14]]
    assert CK.builtin_alignment_heads("large-v3-turbo", 4, 20) == CK.builtin_alignment_heads("turbo", 4, 20)
    assert CK.builtin_alignment_heads("large-v3", 32, 20) == [[7, 0], [10, 17], [12, 18], [13, 12], [16, 1], [17, 14], [19, 11], [21, 4],
                                                               [24, 1], [25, 6]]
    assert CK.builtin_alignment_heads("large", 32, 20) == CK.builtin_alignment_heads("large-v3", 32, 20)


def test_turbo_shaped_checkpoint_loads_with_the_v3_vocabulary(tmp_path):
    tk = WhisperTokenizer.toy([b" b", b"on", b" bon", b"jo", b"ur"], language="fr")
    with open(tmp_path / "multilingual.tiktoken", "wb") as f:
        for tok, rank in tk.ranks.items():
            f.write(base64.b64encode(tok) + b" " + str(rank).encode() + b"\n")
    edims = dict(WW.DIMS["turbo"], n_layer=1)
    tdims = dict(WW.TEXT_DIMS["turbo"], n_vocab=tk.n_vocab + 1, n_text_ctx=32)      # v3: one more language token than the 99-language vocabulary
    enc, dec = WW.synthetic_weights(edims, seed=3), WW.synthetic_decoder_weights(tdims, seed=4)
    np.savez(tmp_path / "turbo.npz", **{"encoder." + k: v.astype(np.float16) for k, v in enc.items()},
             **{"decoder." + k: v.astype(np.float16) for k, v in dec.items()})
    m = CK.load_model("turbo", str(tmp_path))
    assert m.dims == edims and m.text_dims == tdims
    assert sorted(map(tuple, np.argwhere(m.alignment_heads).tolist())) == [(2, 4), (2, 11), (3, 3), (3, 6), (3, 11), (3, 14)]
    assert m.encoder_blob.size == sum(int(np.prod(s)) for _, s in WW.tensor_order(edims))
    tok = CK.load_tokenizer(str(tmp_path), "fr", n_vocab=m.text_dims["n_vocab"])
    assert tok.num_languages == 100 and tok.n_vocab == tdims["n_vocab"]
    # the 100th language shifts every later special token by one: <|startoftranscript|> stays, <|transcribe|> moves
    assert tok.sot == tk.sot and tok.transcribe == tk.transcribe + 1 and tok.timestamp_begin == tk.timestamp_begin + 1
