"""Cost of the string graph next to the trace that feeds it: writes profiles/graph_probe.json.

For every read count (default: the bench set of 10k reads, 10 kb, 15 % error): count, assemble, overlap, align, ONE trace of the passed
pairs with the runs dropped (bella_hip_trace_pairs_flags), graph_add_traced, graph_build with the defaults.  Reported per set: classify,
sort and reduce ms (device time) next to dp_ms and walk_ms of the trace, the edges per second of the reduction, the largest degree and how
many vertices took the over-cap path, and the graph's counts.  The expectation DESIGN.md section 11 checks: the graph costs a small
fraction of the trace."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
from bella_amd import BellaPars, Engine  # noqa: E402
from bella_testkit import synth  # noqa: E402


def probe(nreads, band, repeats):
    rs = synth.make_reads_fast(nreads, read_len=10000, err=0.15, seed=1)
    eng = Engine(0)
    eng.reserve(44 * int(rs.offsets[-1]))
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    npairs, _ = eng.overlap(pars)
    npass = eng.align_pairs(pars)
    t0 = time.time()
    eng.trace_pairs_records(pars, band0=band)
    trace_wall = time.time() - t0
    ts = eng.trace_stats()
    eng.graph_reset()
    t0 = time.time()
    added = eng.graph_add_traced()
    add_s = time.time() - t0
    runs = []
    for _ in range(repeats):                                          # (the first build pays the allocations)
        eng.graph_build()
        runs.append(eng.graph_stats())
    st = min(runs, key=lambda s: s["reduce_ms"])
    out = dict(reads=nreads, bases=int(rs.offsets[-1]), pairs=int(npairs), passed=int(npass), traced=int(ts.pairs), records=int(added),
               trace_dp_ms=ts.dp_ms, trace_walk_ms=ts.walk_ms, trace_total_ms=ts.total_ms, trace_wall_s_python=trace_wall, trace_ops_host_bytes=int(ts.ops_host_bytes),
               add_traced_ms=1e3 * add_s, classify_ms=st["classify_ms"], sort_ms=st["sort_ms"], reduce_ms=st["reduce_ms"], host_ms=st["host_ms"],
               first_build_host_ms=runs[0]["host_ms"], reduce_edges_per_s=st["edges_kept"] / max(1e-9, st["reduce_ms"] / 1e3),
               graph_over_trace=(st["classify_ms"] + st["sort_ms"] + st["reduce_ms"]) / max(1e-9, ts.dp_ms + ts.walk_ms),
               **{k: int(st[k]) for k in ("n_short", "n_internal", "contained_reads", "edges_all", "edges_kept", "edges_reduced", "edges_final", "max_degree",
                                           "overcap_vertices")})
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[10000])
    ap.add_argument("--band", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_probe.json"))
    a = ap.parse_args()
    res = [probe(n, a.band, a.repeats) for n in a.reads]
    for r in res:
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump(dict(sets=res), f, indent=1)
        f.write("\n")
