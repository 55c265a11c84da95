"""The shapes the persistent 256 x 256 GEMM (k_gemm_flat) is tested at, and what each is there for.  tests/test_gemm_flat_host.py asserts on the
CPU that every class claimed here really occurs (gemm_restatement.classify at the MI355X's grid of 256 workgroups); tests/test_gpu_gemm_flat.py
runs them.  The claims are conditions on the inputs: if one fails, the shape changes, not the assertion.

``expect`` keys are those of gemm_restatement.classify; a value is compared for equality, except tiles_per_workgroup (every listed count must
occur on exactly that many workgroups) and the keys in AT_LEAST_ONE (the class must occur: > 0)."""

GRID = 256
AT_LEAST_ONE = ("padding_tiles", "past_the_end", "mixed_workgroups", "padding_then_real", "real_then_padding", "rm_then_vt", "vt_then_rm")

# row-major epilogues (plain, GELU, residual): (M, N, K)
ROW_MAJOR = [
    # one row, one tile, a one-step K loop; 248 workgroups have no tile (and 7 of the other 8 a tile past the list's end)
    dict(shape=(1, 256, 64), expect=dict(rule="default", sm=1, sn=1, nk=1, tiles_per_workgroup={0: 248, 1: 8}, past_the_end=True)),
    # rows around the tile edge; nk = 2
    dict(shape=(255, 256, 128), expect=dict(sm=1, sn=1, nk=2)),
    dict(shape=(256, 256, 128), expect=dict(sm=1, sn=1, nk=2)),
    dict(shape=(257, 512, 128), expect=dict(sm=2, sn=2, nk=2)),
    # the tiles_n == 3 && K <= 1024 walk (sn = 1); nk = 3
    dict(shape=(300, 768, 192), expect=dict(rule="three_short", sm=2, sn=1, nk=3)),
    # tiles_n = 3 with K > 1024: the default walk (sn = 3, sm = 9), entries past the list's end
    dict(shape=(2100, 768, 1088), expect=dict(rule="default", sm=9, sn=3, nk=17, past_the_end=True)),
    # the product's out-projection and fc2 K at the smallest M that still pads the walk
    dict(shape=(2100, 768, 768), expect=dict(rule="three_short", sm=8, sn=1, nk=12, padding_tiles=True)),
    dict(shape=(2100, 768, 3072), expect=dict(rule="default", sm=9, sn=3, nk=48, padding_tiles=True)),
    # F_N_MAX: the widest bias vector behind the ring
    dict(shape=(1300, 6144, 64), expect=dict(rule="default", sm=6, sn=4, nk=1)),
    # tiles_n = 7: sn = 1 by default
    dict(shape=(5300, 1792, 64), expect=dict(rule="default", sm=16, sn=1, nk=1, padding_tiles=True)),
    # the tiles_n == 6 walk; second tiles after an epilogue with nk = 1 (the plain wait counts)
    dict(shape=(8500, 1536, 64), expect=dict(rule="six", sm=16, sn=6, nk=1, tiles_per_workgroup={2: 32, 1: 224}, real_then_padding=True)),
    # 2 tiles on 128 workgroups with nk = 2 (after_stores 1 and 2 in one tile); 20 workgroups mix padding and real tiles, in both orders
    dict(shape=(8448, 2048, 128), expect=dict(rule="default", sm=16, sn=4, nk=2, tiles_per_workgroup={2: 128, 1: 128}, mixed_workgroups=20,
                                               padding_then_real=True, real_then_padding=True)),
    # 3 and 2 tiles per workgroup, nk = 3 (after_stores 1, 2, 0 in turn)
    dict(shape=(16640, 2048, 192), expect=dict(rule="default", sm=16, sn=4, nk=3, tiles_per_workgroup={3: 128, 2: 128}, real_then_padding=True)),
]
GAUSSIAN = [(300, 768, 192), (2100, 768, 768), (2100, 768, 3072), (8448, 2048, 128)]
NO_BIAS = (257, 512, 128)                                   # the one exact case run with bias == nullptr
ROW_COUNT_INDEPENDENCE = [(8448, 2048, 128), (16640, 2048, 192)]       # rows [0, 256) against the same rows run alone with M = 256

# V^T and split forms: (S rows per clip, clips, N, K, split or None, vt_sp); M = S x clips.  rels: the distances rel = S - t_g in (0, 32) that
# vt_store_groups must meet (rel % 8 == 4: the two-8-byte-store path; rel % 8 == 0: a clip boundary on a lane edge)
VT = [
    dict(shape=(256, 5, 512, 128, None, 256), rels=(), expect=dict(nk=2)),                        # clips = tiles: no boundary inside a tile, vt_sp = S
    # the clip boundary moves by 4 positions per tile: every rel in {4, 12, 20, 28} is cut, every rel in {8, 16, 24} a boundary on a lane edge
    dict(shape=(260, 20, 512, 128, None, 272), rels=(4, 8, 12, 16, 20, 24, 28), expect=dict(nk=2)),
    dict(shape=(260, 20, 768, 64, 256, 260), rels=(4, 8, 12, 16, 20, 24, 28), expect=dict(rule="three_short", nk=1)),
    dict(shape=(264, 10, 768, 128, 512, 512), rels=(8, 16, 24), expect=dict(rule="three_short", nk=2)),
    # the product's cross K | V
    dict(shape=(1500, 3, 1536, 768, 768, 1536), rels=(20, 24, 28), expect=dict(rule="six", nk=12)),
    # 432 walk entries on 256 workgroups: a row-major tile and a transposed tile back to back, in both orders
    dict(shape=(1500, 8, 2304, 64, 1536, 1536), rels=(4, 8, 12, 16, 20, 24, 28),
         expect=dict(rule="default", sn=3, nk=1, tiles_per_workgroup={2: 176, 1: 80}, rm_then_vt=True, vt_then_rm=True)),
]

# refused by launch_gemm_flat with PCE_E_LIMIT (-5), nothing launched: (M, N, K, epilogue, rows_per_clip, vt_sp)
REFUSED = [
    (300, 384, 64, 0, 1, 0),                                # N % 256
    (300, 256, 96, 0, 1, 0),                                # K % 64
    (300, 6400, 64, 0, 1, 0),                               # N > F_N_MAX
    (510, 512, 64, 2, 255, 256), (516, 512, 64, 2, 258, 272),            # V^T: S < 256, S % 4
    (510, 512, 64, 256, 255, 256), (516, 512, 64, 256, 258, 272),        # split: the same
    (520, 768, 64, 384, 260, 272),                          # a split that is no multiple of 256
]


def case_id(c):
    return "x".join(str(v) for v in (c["shape"] if isinstance(c, dict) else c) if v is not None)


def check_class(c, expect, what):
    """assert that a gemm_restatement.classify result meets a case's claims"""
    for k, v in expect.items():
        if k == "tiles_per_workgroup":
            assert all(c[k].get(n, 0) == cnt for n, cnt in v.items()), (what, k, c[k])
        elif k in AT_LEAST_ONE and v is True:
            assert c[k] > 0, (what, k, c[k])
        else:
            assert c[k] == v, (what, k, c[k])
