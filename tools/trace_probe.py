"""Speed of the traced alignments next to the X-drop on the same pairs: writes profiles/trace_probe.json.

For every read count (default: the bench sets of 10k and 100k reads, 10 kb, 15 % error): count, assemble, overlap, align, then trace
the passed pairs with the default band.  Reported per set: pairs/s and DP cells/s of the trace (device time of the DP kernels, of the
backtrace kernels, and the whole call with the host staging of the ops), direction bytes, share of extensions repeated with a wider
band, and the X-drop time of the same run (which aligns ALL pairs; the passed share is given; xdrop_cells_same_pairs / dp_cells compares the work on the SAME pairs).
--max-pairs N traces the first N passed pairs through trace_batch instead: the runs are staged on the host (about 9.5 KB per pair
of these reads), so the 100k-read set's tens of millions of passed pairs are sampled, not traced whole."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
from bella_amd import BellaPars, Engine, _lib  # noqa: E402
from bella_testkit import synth  # noqa: E402


def probe(nreads, max_pairs, band):
    rs = synth.make_reads_fast(nreads, read_len=10000, err=0.15, seed=1)
    eng = Engine(0)
    eng.reserve(44 * int(rs.offsets[-1]))
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    npairs, _ = eng.overlap(pars)
    npass = eng.align_pairs(pars)
    xdrop_ms = eng.timings().xdrop_ms
    steps = None
    t0 = time.time()
    if max_pairs and npass > max_pairs:
        pairs, _, _ = eng.get_pairs(ext=False)
        alns = eng.get_alignments()
        pick = np.flatnonzero(alns["passed"])[:max_pairs]
        seeds = np.zeros(len(pick), _lib.SEED_DT)
        for f in ("rid", "cid", "seedH", "seedV"):
            seeds[f] = pairs[f][pick]
        t0 = time.time()
        tr, ops = eng.trace_batch(seeds, alns[pick], pars, band0=band)
        steps = int(alns["steps"][pick].astype(np.int64).sum())
    else:
        tr, ops = eng.trace_pairs(pars, band0=band)
        alns = eng.get_alignments()
        steps = int(alns["steps"][tr["nops"] > 0].astype(np.int64).sum())
        tr = tr[tr["nops"] > 0]
    wall = time.time() - t0
    st = eng.trace_stats()
    out = dict(reads=nreads, pairs=int(npairs), passed=int(npass), traced=int(st.pairs), band0=int(st.band0), xdrop_ms_all_pairs=float(xdrop_ms),
               xdrop_ms_per_pair=float(xdrop_ms) / max(1, npairs), trace_dp_ms=st.dp_ms, trace_walk_ms=st.walk_ms, trace_total_ms=st.total_ms,
               trace_wall_s_python=wall, pairs_per_s_device=st.pairs / max(1e-9, (st.dp_ms + st.walk_ms) / 1e3), pairs_per_s_call=st.pairs / max(1e-9, st.total_ms / 1e3),
               dp_cells=int(st.dp_cells), dp_cells_per_s=st.dp_cells / max(1e-9, st.dp_ms / 1e3), dir_bytes=int(st.dir_bytes), dir_bytes_peak=int(st.dir_bytes_peak),
               batches=int(st.batches), extensions=int(st.extensions), widened_extensions=int(st.widened_extensions),
               repeated_pairs=int(st.repeated_pairs), widened_share=st.widened_extensions / max(1, 2 * st.pairs), pairs_widened=int((tr["widened"] > 0).sum()),
               ops=int(st.ops), ops_per_pair=st.ops / max(1, st.pairs), mean_identity=float((tr["n_eq"] / np.maximum(1, tr["n_eq"] + tr["n_x"] + tr["n_ins"] + tr["n_del"])).mean()),
               trace_ms_per_pair_device=(st.dp_ms + st.walk_ms) / max(1, st.pairs))
    if steps is not None:
        out["xdrop_cells_same_pairs"] = 31 * steps
        out["cell_ratio_same_pairs"] = out["dp_cells"] / max(1, 31 * steps)
    out["trace_over_xdrop_per_pair"] = out["trace_ms_per_pair_device"] / max(1e-12, out["xdrop_ms_per_pair"])
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--max-pairs", type=int, default=0)
    ap.add_argument("--band", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_probe.json"))
    a = ap.parse_args()
    res = [probe(n, a.max_pairs, a.band) for n in a.reads]
    for r in res:
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump(dict(sets=res), f, indent=1)
        f.write("\n")
