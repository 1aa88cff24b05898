"""Speed of the pair alignment (Engine.align_sequences): writes profiles/align_probe.json.

Two inputs: 2,000 pairs of 10 kb at 15 % error in each of the three modes (global: a noisy copy against its template; semi-global: a
noisy copy of 10 kb against a template of 12 kb; dovetail: two reads of 10 kb that share 5 kb), and one global pair of 500 kb at 1 %.
Reported per run: device time of the pack, the DP kernels and the walks, the whole call on the host clock, DP cells and cells per
second of the DP kernels, pairs per second, batches, repeated DPs, pairs by status and the mean identity of the aligned pairs.
tools/trace_probe.py reports the same cells per second for the traced alignments: the two share band.hpp's sweep.

--scoring a,b,o,e: the three 2,000-pair inputs, each aligned with the linear call and then, in the same process,
with the affine one under that scoring; both runs and the ratios affine / linear of dp_ms, walk_ms and cells per second go to
profiles/align_probe_affine.json.  The 500 kb pair is not run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
from bella_amd import Engine  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def genome(n, rng):
    return rng.integers(0, 4, n, dtype=np.uint8)


def noisy(codes, err, rng, mix=(0.10, 0.60, 0.30)):
    """a copy of `codes` (0 .. 3) with substitutions, inserted and deleted bases at `err` per base, split by `mix` (the read generator's)"""
    n = len(codes)
    u = rng.random(n)
    p_sub, p_ins, p_del = (err * m for m in mix)
    dele = u < p_del
    sub = (u >= p_del) & (u < p_del + p_sub)
    ins = (u >= p_del + p_sub) & (u < p_del + p_sub + p_ins)
    b = np.where(sub, (codes + rng.integers(1, 4, n, dtype=np.uint8)) & 3, codes).astype(np.uint8)
    cnt = (~dele).astype(np.int64) + ins
    out = np.repeat(b, cnt)
    at = np.cumsum(cnt)[ins] - 1                                       # an inserted base stands behind its base
    out[at] = rng.integers(0, 4, len(at), dtype=np.uint8)
    return out


def inputs(mode, npairs, length, err, rng):
    seqs, pairs, centre = [], [], []
    for _ in range(npairs):
        if mode == "global":
            T = genome(length, rng)
            Q = noisy(T, err, rng)
            c = (len(T) - len(Q)) // 2
        elif mode == "semiglobal":
            T = genome(length + length // 5, rng)
            a = int(rng.integers(0, length // 5))
            Q = noisy(T[a:a + length], err, rng)
            c = a + (length - len(Q)) // 2                             # the path begins on diagonal a and ends on a + length - len(Q)
        else:
            t = genome(length // 2, rng)
            T = np.concatenate([genome(length - length // 2, rng), noisy(t, err / 2, rng)])
            Q = np.concatenate([noisy(t, err / 2, rng), genome(length - length // 2, rng)])
            c = len(T) - length // 2
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [ACGT[Q].tobytes(), ACGT[T].tobytes()]
        centre.append(c)
    return seqs, pairs, centre


def probe(eng, name, mode, npairs, length, err, band0, band_max, seed, scoring=None):
    rng = np.random.default_rng(seed)
    seqs, pairs, centre = inputs(mode, npairs, length, err, rng)
    kw = {} if scoring is None else dict(scoring=scoring)
    res, ops = eng.align_sequences(seqs, pairs, mode, centre=centre, band0=band0, band_max=band_max, **kw)
    st = eng.align_stats()
    ok = res["status"] == 0
    cols = np.maximum(1, res["n_eq"].astype(np.int64) + res["n_x"] + res["n_ins"] + res["n_del"])
    return dict(name=name, mode=mode, **({} if scoring is None else dict(scoring=list(scoring))), pairs=npairs, length=length, error=err, band0=band0, band_max=band_max, aligned=int(st["aligned"]), band_capped=int(st["band_capped"]),
                too_large=int(st["too_large"]), repeated=int(st["repeated"]), batches=int(st["batches"]), dp_cells=int(st["dp_cells"]), ops=int(st["ops"]),
                pack_ms=st["pack_ms"], dp_ms=st["dp_ms"], walk_ms=st["walk_ms"], total_ms=st["total_ms"], dp_cells_per_s=st["dp_cells"] / max(1e-9, st["dp_ms"] / 1e3),
                pairs_per_s_device=npairs / max(1e-9, (st["pack_ms"] + st["dp_ms"] + st["walk_ms"]) / 1e3), pairs_per_s_call=npairs / max(1e-9, st["total_ms"] / 1e3),
                bands={str(b): int((res["band"] == b).sum()) for b in sorted(set(res["band"].tolist()))},
                mean_identity=float((res["n_eq"][ok] / cols[ok]).mean()) if ok.any() else None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--long", type=int, default=500000)
    ap.add_argument("--band0", type=int, default=512)
    ap.add_argument("--band-max", type=int, default=4096)
    ap.add_argument("--scoring", default=None, help="match,mismatch,gap_open,gap_extend: compare the affine call with the linear one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    scoring = tuple(int(x) for x in a.scoring.split(",")) if a.scoring else None
    if scoring is not None and len(scoring) != 4:
        ap.error("--scoring takes four numbers")
    out = a.out or os.path.join(ROOT, "profiles", "align_probe_affine.json" if scoring else "align_probe.json")
    eng = Engine(0)
    probe(eng, "warm-up", "global", 8, 1000, 0.15, a.band0, a.band_max, 0)
    if scoring is not None:
        probe(eng, "warm-up", "global", 8, 1000, 0.15, a.band0, a.band_max, 0, scoring)
        runs, ratios = [], []
        for k, mode in enumerate(("global", "semiglobal", "dovetail")):
            name = "%d pairs of %d bases at 15 %%" % (a.pairs, a.length)
            lin = probe(eng, name, mode, a.pairs, a.length, 0.15, a.band0, a.band_max, 28 + k)
            aff = probe(eng, name, mode, a.pairs, a.length, 0.15, a.band0, a.band_max, 28 + k, scoring)
            runs += [lin, aff]
            ratios.append(dict(mode=mode, dp_ms=aff["dp_ms"] / lin["dp_ms"], walk_ms=aff["walk_ms"] / lin["walk_ms"],
                               dp_cells_per_s=aff["dp_cells_per_s"] / lin["dp_cells_per_s"], total_ms=aff["total_ms"] / lin["total_ms"]))
        eng.close()
        for r in runs + ratios:
            print(json.dumps(r))
        with open(out, "w") as f:
            json.dump(dict(scoring=list(scoring), runs=runs, affine_over_linear=ratios), f, indent=1)
            f.write("\n")
        sys.exit(0)
    runs = [probe(eng, "%d pairs of %d bases at 15 %%" % (a.pairs, a.length), mode, a.pairs, a.length, 0.15, a.band0, a.band_max, 28 + k)
            for k, mode in enumerate(("global", "semiglobal", "dovetail"))]
    runs.append(probe(eng, "one pair of %d bases at 1 %%" % a.long, "global", 1, a.long, 0.01, a.band0, a.band_max, 31))
    eng.close()
    for r in runs:
        print(json.dumps(r))
    with open(out, "w") as f:
        json.dump(dict(runs=runs), f, indent=1)
        f.write("\n")
