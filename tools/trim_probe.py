"""What coverage trimming costs and what it mends: writes profiles/trim_probe.json.

For every read count (default: the 2,000 x 10 kb and the 10k-read sets, 15 % error): 30 % of the reads get 1,200 to 3,000 random bases in
front, 30 % behind, and one chimera per 100 reads is added -- two reads drawn at random joined end to end (at 30x two random reads of a
set overlap with probability below 1 %) -- all from a fixed seed.  Then count, assemble, overlap, align, ONE trace with the runs
dropped, graph_add_traced, and the graph twice: as the code stood (graph_build, graph_clean, graph_unitigs) and with graph_trim in front.
Reported per set: events, sort and sweep ms of the trim next to classify_ms + sort_ms + reduce_ms of the build, the trim's counts, and for
both graphs INTERNAL records, components, unitigs, N50 and the largest unitig.  Figures are recorded, not asserted.

--clip-ends: the same pairs are traced once more with every alignment clipped at --clip-identity, and both graphs
are built again from the clipped records; the set's entry keeps under "clip_ends" the clip's statistics, clip_ms next to walk_ms of both
traces (the clipped one runs the writing walk, which the records alone do not need), and the same figures: junk bases the trim removes,
chimeras with two regions, INTERNAL records, unitigs, N50."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import numpy as np  # noqa: E402
from bella_amd import BellaPars, Engine  # noqa: E402
from bella_testkit import graph_mirror as G  # noqa: E402
from bella_testkit import synth  # noqa: E402
from bella_testkit import unitig_mirror as U  # noqa: E402


def spoil(rs, seed, frac=0.3, lo=1200, hi=3000, chimera_every=100):
    """-> (ReadSet with junk ends and chimeras, number of reads with junk, number of chimeras, junk bases)"""
    rng = np.random.default_rng(seed)
    seqs = rs.seqs()
    n = len(seqs)
    head = np.where(rng.random(n) < frac, rng.integers(lo, hi + 1, n), 0)
    tail = np.where(rng.random(n) < frac, rng.integers(lo, hi + 1, n), 0)
    out = [U.random_genome(int(h), seed + 2 * i + 1) + s + U.random_genome(int(t), seed + 2 * i + 2) for i, (s, h, t) in enumerate(zip(seqs, head, tail))]
    nch = n // chimera_every
    for _ in range(nch):
        a, b = (int(x) for x in rng.integers(0, n, 2))
        out.append((seqs[a] + seqs[b])[:65000])
    return synth.ReadSet.from_strings(out), int(((head > 0) | (tail > 0)).sum()), nch, int(head.sum() + tail.sum())


def graph_figures(eng, nreads):
    st = eng.graph_stats()
    off, e, cont = eng.graph()
    comp = G.components(nreads, e, cont != 0)
    eng.graph_clean()
    eng.graph_unitigs()
    us = eng.unitig_stats()
    return dict(n_internal=int(st["n_internal"]), n_short=int(st["n_short"]), contained_reads=int(st["contained_reads"]), uncovered_reads=int((cont == 2).sum()),
                edges_final=int(st["edges_final"]), components=comp, unitigs=int(us["unitigs"]), n50=int(us["n50"]), largest=int(us["largest"]),
                total_bases=int(us["total_bases"]), classify_ms=st["classify_ms"], sort_ms=st["sort_ms"], reduce_ms=st["reduce_ms"])


def trimmed_figures(eng, rs, nch, repeats):
    """after graph_add_traced: the untrimmed graph, the trim (best of `repeats`), the trimmed graph"""
    eng.graph_build()
    plain = graph_figures(eng, rs.nreads)
    runs = []
    for _ in range(repeats):
        eng.graph_trim()
        runs.append(eng.trim_stats())
    ts = min(runs, key=lambda s: s["events_ms"] + s["sort_ms"] + s["sweep_ms"])
    clips = eng.graph_clips()
    eng.graph_build()
    outside = eng.trim_stats()["records_outside"]
    trimmed = graph_figures(eng, rs.nreads)
    chim = clips[rs.nreads - nch:] if nch else clips[:0]
    return dict(chimeras_split=int((chim["nregions"] >= 2).sum()), records_outside=int(outside), junk_bases_removed=int(ts["bases_before"]) - int(ts["bases_after"]),
                **{k: int(ts[k]) for k in ("intervals", "reads_clipped", "reads_uncovered", "reads_multi", "bases_before", "bases_after")},
                untrimmed=plain, trimmed=trimmed)


def probe(nreads, seed, repeats, clip_identity=None):
    rs, njunk, nch, junk_bases = spoil(synth.make_reads_fast(nreads, read_len=10000, err=0.15, seed=1), seed)
    eng = Engine(0)
    eng.reserve(44 * int(rs.offsets[-1]))
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    npairs, _ = eng.overlap(pars)
    npass = eng.align_pairs(pars)
    eng.trace_pairs_records(pars)
    walk_plain = eng.trace_stats().walk_ms
    eng.graph_reset()
    added = eng.graph_add_traced()
    eng.graph_build()
    plain = graph_figures(eng, rs.nreads)
    runs = []
    for _ in range(repeats):                                          # (the first trim pays the allocations)
        eng.graph_trim()
        runs.append(eng.trim_stats())
    ts = min(runs, key=lambda s: s["events_ms"] + s["sort_ms"] + s["sweep_ms"])
    clips = eng.graph_clips()
    eng.graph_build()
    outside = eng.trim_stats()["records_outside"]
    trimmed = graph_figures(eng, rs.nreads)
    chim = clips[rs.nreads - nch:] if nch else clips[:0]
    out = dict(reads=rs.nreads, bases=int(rs.offsets[-1]), reads_with_junk=njunk, chimeras=nch, chimeras_split=int((chim["nregions"] >= 2).sum()), pairs=int(npairs),
               passed=int(npass), records=int(added), trim_events_ms=ts["events_ms"], trim_sort_ms=ts["sort_ms"], trim_sweep_ms=ts["sweep_ms"], trim_host_ms=ts["host_ms"],
               first_trim_host_ms=runs[0]["host_ms"], build_ms=trimmed["classify_ms"] + trimmed["sort_ms"] + trimmed["reduce_ms"],
               trim_over_build=(ts["events_ms"] + ts["sort_ms"] + ts["sweep_ms"]) / max(1e-9, trimmed["classify_ms"] + trimmed["sort_ms"] + trimmed["reduce_ms"]),
               records_outside=int(outside), **{k: int(ts[k]) for k in ("intervals", "reads_clipped", "reads_uncovered", "reads_multi", "bases_before", "bases_after")},
               untrimmed=plain, trimmed=trimmed)
    out["junk_bases"] = junk_bases
    if clip_identity:
        eng.trace_pairs_records(pars, clip=clip_identity)
        tst, ks = eng.trace_stats(), eng.clip_stats()
        eng.graph_reset()
        nrec = eng.graph_add_traced()
        out["clip_ends"] = dict(identity=clip_identity, records=int(nrec), clip_ms=ks["clip_ms"], walk_ms=tst.walk_ms, walk_ms_without_clip=walk_plain, dp_ms=tst.dp_ms,
                                clip_stats={k: int(v) for k, v in ks.items() if k not in ("clip_ms", "pad")}, **trimmed_figures(eng, rs, nch, repeats))
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[2000, 10000])
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clip-ends", action="store_true")
    ap.add_argument("--clip-identity", type=int, default=650)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trim_probe.json"))
    a = ap.parse_args()
    res = [probe(n, a.seed, a.repeats, a.clip_identity if a.clip_ends else None) for n in a.reads]
    for r in res:
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump(dict(sets=res), f, indent=1)
        f.write("\n")
