"""The batches of tests/test_lufs_host.py and tests/test_gpu_lufs_stages.py: clips, slices and what each batch is there for, and the loop that holds a
run's stages (from ``ProsodyEngine.lufs_fetch_stages`` or from ``emulate_batch``) against tests/lufs_restatement.py slice by slice."""
import math

import numpy as np

from tests import lufs_restatement as R


def signal(kind, n, rate, seed=0):
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n) / rate
    if kind == "tone20":                                     # noise on a 20 Hz tone: what the high-pass stresses most
        v = 14000 * np.sin(2 * np.pi * 20.0 * t) + 3000 * rng.standard_normal(n)
    elif kind == "min":                                      # a clip that holds -32768
        v = 9000 * rng.standard_normal(n); v[n // 3] = -32768
    elif kind == "square":
        v = np.where(np.floor(t * 200.0) % 2 == 0, 32767, -32767)
    elif kind == "const":
        v = np.full(n, 12345)
    elif kind in ("gate_abs", "gate_rel", "gate_both"):
        loud = 9000 * rng.standard_normal(n)
        quiet = loud * 10 ** (-15 / 20)                      # 15 dB down: over the absolute gate, under the relative one
        lsb = rng.integers(1, 4, n) * rng.choice([-1, 1], n)  # 1 .. 3 LSB under a full-scale peak: under the absolute gate
        a, b = int(0.5 * n), int(0.75 * n)
        v = loud.copy()
        if kind == "gate_abs":
            v[a:] = lsb[a:]
        elif kind == "gate_rel":
            v[a:] = quiet[a:]
        else:
            v[a:b] = quiet[a:b]; v[b:] = lsb[b:]
        v[7] = 32767
    else:
        raise KeyError(kind)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def one_block(rate):
    return math.ceil(0.4 * rate)


def batches():
    """name -> dict(rate, meter (0: the data's), clips, slices [(clip, begin, end)], wants: the edges the batch must show)."""
    B = {}
    r = 16000
    clips = [signal("const", 777, r), signal("tone20", 9001, r, 1), signal("min", 8003, r, 2), signal("square", 7001, r), signal("const", 6503, r),
             signal("tone20", 7429, r, 3)]
    assert sum(len(c) for c in clips) % 8 != 0
    sl = [(1, k, k + 6400 + 13 * k) for k in range(8)]        # clip 1 starts at 777: the eight begin residues
    sl += [(1, -100, 6500),                                   # begins before its clip
           (2, 0, 0),                                         # empty
           (1, 2000, 9001 + 200),                             # ends past it
           (2, 10, 10 + 6399),                                # one sample too short, between live neighbours
           (1, 9001 + 50, 9001 + 50 + 6400),                  # wholly outside: over the next clip's samples in the buffer, all zeros by the mask
           (2, 0, 6400),                                      # exactly one block
           (2, 100, 100 + 7425),                              # 2 blocks, 31 chunks, one of length 1
           (3, 0, 0), (3, 0, 7001), (4, 0, 6503),
           (0, 0, 777),                                       # too short
           (5, 0, 7429)]                                      # ends at the very end of the resident buffer
    B["addresses_16k"] = dict(rate=r, meter=0, clips=clips, slices=sl)
    for r in (8000, 11025, 22050, 44100, 48000):
        n1 = one_block(r)
        clips = [signal("min", 333, r), signal("tone20", int(0.95 * r) + 1, r, r % 97)]
        sl = [(1, 3, 3 + n1), (1, 5, 5 + n1 - 1), (1, 0, len(clips[1])), (1, 2, 2 + n1 + r // 10)]
        if r == 8000:
            clips += [signal("tone20", 3713, r, 5)] + [signal(k, 20000, r, 6 + i) for i, k in enumerate(("gate_abs", "gate_rel", "gate_both"))]
            sl += [(2, 0, 3200), (2, 1, 1 + 3601), (2, 0, 3713), (3, 0, 20000), (4, 0, 20000), (5, 0, 20000)]   # 13, 16, 17 chunks; the gates
        B[f"short_{r}"] = dict(rate=r, meter=0, clips=clips, slices=sl)
    B["long_44100"] = dict(rate=44100, meter=0, clips=[signal("min", 5, 44100), signal("tone20", 251057, 44100, 11)],
                           slices=[(1, 0, 250801), (1, 0, 251057)])                      # 1024 and 1025 chunks
    B["long_48000"] = dict(rate=48000, meter=0, clips=[signal("tone20", 258753 + 3, 48000, 12)],
                           slices=[(0, 3, 3 + 258497), (0, 0, 258753)])                  # 1024 and 1025 chunks
    B["blocks_16k"] = dict(rate=16000, meter=0, clips=[signal("min", 108001, 16000, 13)],
                           slices=[(0, 0, 106401), (0, 0, 108001)])                      # 64 and 65 gating blocks
    B["meter_44100_on_16k"] = dict(rate=16000, meter=44100, clips=[signal("tone20", 19201, 16000, 14), signal("min", 40001, 16000, 15)],
                                   slices=[(0, 0, 19201), (0, 0, 17639), (1, 1, 40001), (0, 1, 1 + 17640)])
    return B


# the edges every batch must show, in the counts of check_batch
WANTS = {"addresses_16k": lambda c: c["residues"] == set(range(8)) and c["len1"] and c["before"] and c["past"] and c["outside"] == 1 and c["buffer_end"]
         and c["too_short"] == 2 and c["empty"] == 2 and c["one_block"] >= 2,
         "short_8000": lambda c: c["lt_group"] and c["chunks16"] and c["chunks17"] and c["absolute"] == 2 and c["relative"] == 2 and c["too_short"] == 1,
         "long_44100": lambda c: c["chunks1024"] == 1 and c["chunks1025"] == 1, "long_48000": lambda c: c["chunks1024"] == 1 and c["chunks1025"] == 1,
         "blocks_16k": lambda c: c["blocks64"] == 1 and c["blocks65"] == 1, "meter_44100_on_16k": lambda c: c["too_short"] == 1 and c["one_block"] >= 1}


def wanted(name, cnt):
    return bool(WANTS.get(name, lambda c: c["one_block"] >= 1 and c["too_short"] == 1)(cnt))


def buffer_of(batch):
    off = np.concatenate([[0], np.cumsum([len(c) for c in batch["clips"]])]).astype(np.int64)
    return np.concatenate(batch["clips"]), off


def emulate_batch(batch, mutation=None, only=None):
    """What ``lufs_fetch_stages`` and ``lufs`` return, from the float64 emulation of the kernels (``only``: mutate this slice alone)."""
    rate = batch["meter"] or batch["rate"]
    coef = R.kweight_float64(rate)
    pcm, off = buffer_of(batch)
    chunks, blocks, slices, lufs, status = [], [], [], [], []
    apow = R.powers_float64(coef)
    for i, (c, b, e) in enumerate(batch["slices"]):
        pl = R.plan(e - b, rate)
        status.append(pl["status"])
        g = off[c] + b + np.arange(e - b)
        real = (g >= off[c]) & (g < off[c + 1])
        peak = R.peak_of(pcm[g[real]].astype(np.int64)) if real.any() else 1
        row = dict(first_chunk=sum(len(x["rel"]) for x in chunks), first_block=sum(len(x["c0"]) for x in blocks), status=pl["status"], peak=peak)
        if pl["status"] != R.OK:
            lufs.append(np.nan); slices.append(dict(row, n_chunks=0, n_blocks=0)); continue
        st, v, pk = R.emulate(coef, rate, pcm, int(off[c]), int(off[c + 1]), int(off[c] + b), int(off[c] + e),
                              mutation if only is None or only == i else None)
        assert pk == peak
        if mutation == "table_entry":
            apow = st["apow"]
        chunks.append(st); blocks.append(st); lufs.append(v)
        slices.append(dict(row, n_chunks=len(st["rel"]), n_blocks=len(st["c0"])))
    from prosody_control_french_tts_amd import engine as E
    ch = np.zeros(sum(len(x["rel"]) for x in chunks), E.LUFS_CHUNK_DTYPE)
    bl = np.zeros(sum(len(x["c0"]) for x in blocks), E.LUFS_BLOCK_DTYPE)
    sr = np.zeros(len(slices), E.LUFS_SLICE_DTYPE)
    live = iter(chunks)
    for i, row in enumerate(slices):
        for k, v in row.items():
            sr[i][k] = v
        if row["status"] == R.OK:
            st = next(live)
            a = slice(row["first_chunk"], row["first_chunk"] + row["n_chunks"]); q = slice(row["first_block"], row["first_block"] + row["n_blocks"])
            ch["rel"][a] = st["rel"]; ch["len"][a] = st["len"]; ch["slice"][a] = i
            ch["state_end"][a] = st["state_end"]; ch["state_init"][a] = st["state_init"]; ch["energy"][a] = st["energy"]
            bl["c0"][q] = st["c0"]; bl["c1"][q] = st["c1"]; bl["z"][q] = st["z"]
    return dict(coef=coef, apow=apow, chunks=ch, slices=sr, blocks=bl), np.array(lufs), np.array(status, np.int32)


_TABLES = {}


def tables(coef):
    key = np.asarray(coef, np.float64).tobytes()
    if key not in _TABLES:
        _TABLES[key] = R.Tables(coef)
    return _TABLES[key]


def check_batch(batch, stages, lufs, status):
    """Every slice of a run against the restatement -> (worst ratio per stage, counts of the edges seen, the list of failures as text)."""
    rate = batch["meter"] or batch["rate"]
    pcm, off = buffer_of(batch)
    fails, worst = [], {}
    cnt = dict(len1=0, chunks1024=0, chunks1025=0, blocks64=0, blocks65=0, residues=set(), absolute=0, relative=0, too_short=0, empty=0, outside=0,
               one_block=0, lt_group=0, chunks16=0, chunks17=0, before=0, past=0, buffer_end=0, log10_ulps=0.0, block_rel=0.0, margin=np.inf, live=0)
    coef = np.asarray(stages["coef"], np.float64)
    if not np.array_equal(coef, R.kweight_float64(rate)):
        # the design is host libm against numpy's: a last-place difference is no error of the kernels; the stages below take the fetched numbers
        rel = np.max(np.abs(coef - R.kweight_float64(rate)) / np.abs(R.kweight_float64(rate)))
        if rel > 8 * 2.0 ** -52:
            fails.append(f"coefficients off the float64 design by {rel:.3g} relative")
    tab = tables(coef)
    worst["table"] = tab.table_ratio(stages["apow"])
    if not worst["table"] <= 1.0:
        fails.append(f"power table: |got - want| / bound = {worst['table']:.4g}")
    if not np.array_equal(np.asarray(stages["apow"], np.float64).reshape(-1, 4, 4), R.powers_float64(coef)):
        fails.append("power table differs from transition_powers' float64 arithmetic")
    sr, ch, bl = stages["slices"], stages["chunks"], stages["blocks"]
    nch = nbl = 0
    for i, (c, b, e) in enumerate(batch["slices"]):
        pl = R.plan(e - b, rate)
        row = sr[i]
        if (row["first_chunk"], row["first_block"], row["status"]) != (nch, nbl, pl["status"]) or status[i] != pl["status"]:
            fails.append(f"slice {i}: first_chunk / first_block / status {row} want {(nch, nbl, pl['status'])}")
            break
        clip = batch["clips"][c]
        raw = R.slice_samples(clip, b, e)
        if row["peak"] != R.peak_of(raw):
            fails.append(f"slice {i}: peak {row['peak']} want {R.peak_of(raw)}")
        if pl["status"] != R.OK:
            cnt["too_short" if pl["status"] == R.TOO_SHORT else "empty"] += 1
            if row["n_chunks"] or row["n_blocks"] or not np.isnan(lufs[i]):
                fails.append(f"slice {i}: a slice without blocks has chunks, blocks or a value")
            continue
        a = slice(nch, nch + row["n_chunks"]); q = slice(nbl, nbl + row["n_blocks"])
        nch += row["n_chunks"]; nbl += row["n_blocks"]
        if row["n_chunks"] != len(pl["rel"]) or row["n_blocks"] != len(pl["c0"]) or not np.all(ch["slice"][a] == i):
            fails.append(f"slice {i}: {row['n_chunks']} chunks, {row['n_blocks']} blocks, want {len(pl['rel'])}, {len(pl['c0'])}")
            break
        st = dict(apow=np.asarray(stages["apow"]).reshape(-1, 4, 4), rel=ch["rel"][a], len=ch["len"][a], state_end=ch["state_end"][a],
                  state_init=ch["state_init"][a], energy=ch["energy"][a], c0=bl["c0"][q], c1=bl["c1"][q], z=bl["z"][q])
        x = raw.astype(np.float64) / np.float64(row["peak"])
        o = R.check_slice(tab, rate, x, st, lufs[i])
        for k in ("tables_equal", "tiles", "covers"):
            if not o[k]:
                fails.append(f"slice {i}: {k} is false")
        if "ratios" not in o:
            continue
        for k in ("init0_zero", "z_equal"):
            if not o[k]:
                fails.append(f"slice {i}: {k} is false")
        if o.get("lufs_equal_inf") is False:
            fails.append(f"slice {i}: {lufs[i]} for an all-zero slice")
        for k, v in o["ratios"].items():
            if v is not None:
                worst[k] = max(worst.get(k, 0.0), v)
                if not v <= 1.0:
                    fails.append(f"slice {i}: stage {k}: |got - want| / bound = {v:.4g}")
        if not np.any(raw):
            cnt["outside"] += 1
        elif o["margin"] < 1e-6:
            fails.append(f"slice {i}: a block lies {o['margin']:.3g} LU from a threshold")
        else:
            cnt["margin"] = min(cnt["margin"], o["margin"])
        n = o["n_chunks"]
        cnt["live"] += 1
        cnt["len1"] += int(o["min_len"] == 1); cnt["chunks1024"] += n == 1024; cnt["chunks1025"] += n == 1025
        cnt["chunks16"] += n == 16; cnt["chunks17"] += n == 17; cnt["lt_group"] += n < R.GROUP
        cnt["blocks64"] += o["n_blocks"] == 64; cnt["blocks65"] += o["n_blocks"] == 65; cnt["one_block"] += o["n_blocks"] == 1
        cnt["residues"].add(int((off[c] + b) % 8))
        cnt["before"] += b < 0 < e; cnt["past"] += b < len(clip) < e; cnt["buffer_end"] += off[c] + e == off[-1]
        if np.any(raw):
            cnt["absolute"] += o["absolute_dropped"] > 0; cnt["relative"] += o["relative_dropped"] > 0
        cnt["log10_ulps"] = max(cnt["log10_ulps"], o.get("log10_ulps", 0.0)); cnt["block_rel"] = max(cnt["block_rel"], o["block_rel"])
    if not fails and (nch, nbl) != (len(ch), len(bl)):
        fails.append(f"{len(ch)} chunks and {len(bl)} blocks fetched, the slices hold {nch} and {nbl}")
    return worst, cnt, fails
