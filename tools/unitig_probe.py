"""Cost and outcome of tip clipping, bubble popping, unitig compaction and the sequence gather next to the graph build that feeds them:
writes profiles/unitig_probe.json.

For every set (default: 2,000 x 10 kb and the bench set of 10k reads, both at 15 % error): count, assemble, overlap, align, one trace
that votes into the pileup table (the runs are not staged), graph_add_traced, graph_build, graph_clean, graph_unitigs, all with the defaults.  Reported per set: reads removed
per round, unitigs, largest unitig, N50 and their total length against the genome's, the clean, rank and gather timers (the first two
span the host's read-backs: bella_unitig_stats in include/bella_hip.h) next to the build's classify + sort + reduce of the same run,
and the gather's bytes over its time (one byte written per base, a quarter byte read).  Then the same with graph_pop_bubbles between the
clean and the unitigs: sources / found / popped / reads removed per round, pop_ms, and unitigs, largest and N50
with the stage next to those without it.  Last, the unitig consensus of those unitigs: decide_ms and write_ms (one
launch each), the table bytes the decision read over its time, and the unitigs' total length raw and polished against the genome span."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
from bella_amd import BellaPars, Engine  # noqa: E402
from bella_testkit import synth  # noqa: E402


def probe(nreads, seed, repeats, fast):
    rs = (synth.make_reads_fast if fast else synth.make_reads)(nreads, read_len=10000, err=0.15, seed=seed)
    meta = [[int(x) for x in n.split("_")[1:]] for n in rs.names]     # (start, length, strand)
    span = max(m[0] + m[1] for m in meta) - min(m[0] for m in meta)
    eng = Engine(0)
    eng.reserve(44 * int(rs.offsets[-1]))
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    eng.align_pairs(pars)
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    eng.graph_reset()
    eng.graph_add_traced()
    runs = []
    for _ in range(repeats):                                          # (the first run pays the allocations)
        eng.graph_build()
        gs = eng.graph_stats()
        eng.graph_clean()
        eng.graph_unitigs()
        us = eng.unitig_stats()
        eng.graph_build()
        eng.graph_clean()
        eng.graph_pop_bubbles()
        bs = eng.bubble_stats()
        eng.graph_unitigs()
        eng.graph_polish_unitigs()
        runs.append((gs, us, bs, eng.unitig_stats(), eng.polish_stats()))
    gs, us, _, _, _ = min(runs, key=lambda r: r[1]["rank_ms"] + r[1]["gather_ms"])
    _, _, bs, ps, _ = min(runs, key=lambda r: r[2]["pop_ms"])
    pol = min((r[4] for r in runs), key=lambda q: q["decide_ms"] + q["write_ms"])
    build_ms = gs["classify_ms"] + gs["sort_ms"] + gs["reduce_ms"]
    out = dict(reads=nreads, bases=int(rs.offsets[-1]), genome_span=int(span), edges_final=int(gs["edges_final"]), contained_reads=int(gs["contained_reads"]),
               tips_per_round=us["tips_per_round"], reads_per_round=us["reads_per_round"], reads_removed=int(us["reads_removed"]), edges_removed=int(us["edges_removed"]),
               unitigs=int(us["unitigs"]), circular=int(us["circular"]), links=int(us["links"]), largest=int(us["largest"]), n50=int(us["n50"]),
               total_bases=int(us["total_bases"]), total_over_span=us["total_bases"] / max(1, span), rank_rounds=int(us["rank_rounds"]),
               clean_ms=us["clean_ms"], rank_ms=us["rank_ms"], gather_ms=us["gather_ms"], build_ms=build_ms,
               unitigs_over_build=(us["clean_ms"] + us["rank_ms"] + us["gather_ms"]) / max(1e-9, build_ms),
               gather_bytes=int(us["gather_bytes"] * 5 // 4), gather_gb_per_s=us["gather_bytes"] * 1.25 / max(1e-9, us["gather_ms"] * 1e6))
    out["pop"] = dict(rounds=int(bs["rounds"]), sources=bs["sources"], found=bs["found"], popped=bs["popped"], reads_per_round=bs["reads_per_round"],
                      edges_per_round=bs["edges_per_round"], reads_removed=int(bs["reads_removed"]), edges_removed=int(bs["edges_removed"]), pop_ms=bs["pop_ms"],
                      pop_over_build=bs["pop_ms"] / max(1e-9, build_ms), unitigs=int(ps["unitigs"]), largest=int(ps["largest"]), n50=int(ps["n50"]),
                      total_bases=int(ps["total_bases"]), unitigs_without=int(us["unitigs"]), largest_without=int(us["largest"]), n50_without=int(us["n50"]))
    out["polish"] = dict(min_depth=int(pol["min_depth"]), unitigs=int(pol["unitigs"]), vertices=int(pol["vertices"]), tiles=int(pol["tiles"]),
                         bases_before=int(pol["bases_before"]), bases_after=int(pol["bases_after"]), before_over_span=pol["bases_before"] / max(1, span),
                         after_over_span=pol["bases_after"] / max(1, span), substituted=int(pol["substituted"]), deleted=int(pol["deleted"]),
                         inserted=int(pol["inserted"]), covered=int(pol["covered"]), decide_ms=pol["decide_ms"], write_ms=pol["write_ms"],
                         gather_ms=ps["gather_ms"], table_bytes=int(pol["table_bytes"]),
                         decide_gb_per_s=(pol["table_bytes"] + pol["bases_before"]) / max(1e-9, pol["decide_ms"] * 1e6),
                         write_gb_per_s=(pol["bases_before"] + pol["bases_after"]) / max(1e-9, pol["write_ms"] * 1e6))
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["2000:21:exact", "10000:1:fast"], help="reads:seed:exact|fast (the generator: synth.make_reads / make_reads_fast)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitig_probe.json"))
    a = ap.parse_args()
    res = []
    for s in a.sets:
        n, seed, gen = s.split(":")
        res.append(probe(int(n), int(seed), a.repeats, gen == "fast"))
        print(json.dumps(res[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(sets=res), f, indent=1)
        f.write("\n")
