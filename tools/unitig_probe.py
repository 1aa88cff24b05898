"""Cost and outcome of tip clipping, bubble popping, unitig compaction and the sequence gather next to the graph build that feeds them:
writes profiles/unitig_probe.json.

For every set (default: 2,000 x 10 kb and the bench set of 10k reads, both at 15 % error): count, assemble, overlap, align, one trace
that votes into the pileup table (the runs are not staged), graph_add_traced, graph_build, graph_clean, graph_unitigs, all with the defaults.  Reported per set: reads removed
per round, unitigs, largest unitig, N50 and their total length against the genome's, the clean, rank and gather timers (the first two
span the host's read-backs: bella_unitig_stats in include/bella_hip.h) next to the build's classify + sort + reduce of the same run,
and the gather's bytes over its time (one byte written per base, a quarter byte read).  Then the same with graph_pop_bubbles between the
clean and the unitigs: sources / found / popped / reads removed per round, pop_ms, and unitigs, largest and N50
with the stage next to those without it.  Last, the unitig consensus of those unitigs: decide_ms and write_ms (one
launch each), the table bytes the decision read over its time, and the unitigs' total length raw and polished against the genome span.
--cut-weak: one more pass per repeat -- build, clean, pop, then the command line's weak-overlap schedule (cuts at 500,
600 and 700 permille, tips and bubbles again after a cut that took an edge), unitigs -- and per set the edges cut, forks and weak edges per
step, cut_ms per step next to clean_ms and pop_ms of the same run, and unitigs, largest and N50 with the schedule next to those without.
--polish-rounds N: N - 1 realignment rounds after the polish, and per round the reads by status, place_ms, dp_ms,
walk_ms, vote_ms and decide_ms next to the first trace's dp_ms of the same set, the DP cells, the batches and the length after the round.
--align-links: the links aligned on the newest sequences, written to profiles/links_probe.json: the links by status,
the distribution of ovl_a - oa (found against expected overlap, in current coordinates) and of the identity over the ALIGNED links,
pack_ms, dp_ms, walk_ms and the DP's cell updates per second next to the last realignment round's k_rea_dp of the same run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
from bella_amd import BellaPars, Engine  # noqa: E402
from bella_testkit import links_mirror, synth  # noqa: E402


WEAK_RATIOS = (500, 600, 700)                                         # bella-hip --cut-weak's defaults: --weak-min 500 --weak-max 700 --weak-steps 2


def weak_pass(eng):
    """build, clean, pop, the schedule, unitigs: -> dict of the pass's figures"""
    eng.graph_build()
    eng.graph_clean()
    clean_ms = eng.unitig_stats()["clean_ms"]
    eng.graph_pop_bubbles()
    pop_ms = eng.bubble_stats()["pop_ms"]
    steps = []
    for r in WEAK_RATIOS:
        eng.graph_cut_weak(ratio_permille=r)
        ws = eng.weak_stats()
        step = dict(ratio_permille=r, forks=int(ws["forks"]), weak=int(ws["weak"]), edges_cut=int(ws["edges_removed"]), cut_ms=ws["cut_ms"], reads_clipped_after=0, bubbles_popped_after=0)
        if ws["edges_removed"]:
            eng.graph_clean()
            step["reads_clipped_after"] = int(eng.unitig_stats()["reads_removed"])
            eng.graph_pop_bubbles()
            step["bubbles_popped_after"] = int(sum(eng.bubble_stats()["popped"]))
        steps.append(step)
    eng.graph_unitigs()
    us = eng.unitig_stats()
    return dict(steps=steps, edges_cut=sum(x["edges_cut"] for x in steps), cut_ms=sum(x["cut_ms"] for x in steps), clean_ms=clean_ms, pop_ms=pop_ms,
                unitigs=int(us["unitigs"]), largest=int(us["largest"]), n50=int(us["n50"]), total_bases=int(us["total_bases"]))


def realign_rounds(eng, rounds):
    """rounds - 1 realignment rounds on the polish the context holds: -> one dict per round"""
    out = []
    for _ in range(max(0, rounds - 1)):
        eng.graph_realign_unitigs()
        st = eng.realign_stats()
        out.append({k: (float(v) if k.endswith("_ms") else int(v)) for k, v in st.items()})
    return out


def dist(values):
    """min, 10 %, median, 90 %, max and mean of a list of numbers (None when it is empty)"""
    if not len(values):
        return None
    v = np.sort(np.asarray(values, np.float64))
    q = lambda f: float(v[min(len(v) - 1, int(f * len(v)))])
    return dict(n=len(v), min=float(v[0]), p10=q(0.1), median=q(0.5), p90=q(0.9), max=float(v[-1]), mean=float(v.mean()))


def align_links(eng, u, cur, rea):
    """the links aligned on the sequences the context holds (cur: what the polish or the last round returned; None: raw) -> dict"""
    eng.graph_align_links()
    st = eng.link_stats()
    alns, _ = eng.link_alignments()
    al = np.flatnonzero(alns["status"] == links_mirror.ALIGNED)
    shift = [int(alns[k]["ovl_a"]) - links_mirror.expected(u, cur, int(k))[0] for k in al]
    cols = (alns["n_eq"] + alns["n_x"] + alns["n_ins"] + alns["n_del"]).astype(np.int64)
    out = {k: (float(v) if k.endswith("_ms") else int(v)) for k, v in st.items() if k != "pad"}
    out.update(found_minus_expected=dist(shift), identity_permille=dist((1000 * alns["n_eq"][al].astype(np.int64) // np.maximum(cols[al], 1)).tolist()),
               cells_per_s=st["dp_cells"] / max(1e-9, st["dp_ms"] * 1e-3))
    if rea:
        out.update(realign_dp_ms=rea[-1]["dp_ms"], realign_dp_cells=rea[-1]["dp_cells"], realign_cells_per_s=rea[-1]["dp_cells"] / max(1e-9, rea[-1]["dp_ms"] * 1e-3))
    return out


def probe(nreads, seed, repeats, fast, cut_weak=False, polish_rounds=1, links=False):
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
    trace_dp_ms = eng.trace_stats().dp_ms
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
        u = eng.graph_unitigs()
        cur = eng.graph_polish_unitigs()
        pst = eng.polish_stats()
        rea = realign_rounds(eng, polish_rounds)
        lnk = align_links(eng, u, eng.realigned() if rea else cur, rea) if links else None
        runs.append((gs, us, bs, eng.unitig_stats(), pst, weak_pass(eng) if cut_weak else None, rea, lnk))
    gs, us = min(runs, key=lambda r: r[1]["rank_ms"] + r[1]["gather_ms"])[:2]
    bs, ps = min(runs, key=lambda r: r[2]["pop_ms"])[2:4]
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
    if cut_weak:                                                      # (the unitigs "without" are the pop pass's: clean and pop, no schedule)
        out["weak"] = dict(min((r[5] for r in runs), key=lambda w: w["cut_ms"]), unitigs_without=int(ps["unitigs"]), largest_without=int(ps["largest"]), n50_without=int(ps["n50"]))
    if polish_rounds > 1:                                             # (the run whose first round's DP was the fastest)
        out["realign"] = dict(rounds=min((r[6] for r in runs), key=lambda q: q[0]["dp_ms"]), trace_dp_ms=trace_dp_ms, genome_span=int(span))
    if links:                                                         # (the run whose link DP was the fastest)
        out["links"] = min((r[7] for r in runs), key=lambda q: q["dp_ms"])
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["2000:21:exact", "10000:1:fast"], help="reads:seed:exact|fast (the generator: synth.make_reads / make_reads_fast)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitig_probe.json"))
    ap.add_argument("--cut-weak", action="store_true", help="also run the weak-overlap schedule after the clean and the pop (DESIGN.md section 17)")
    ap.add_argument("--polish-rounds", type=int, default=1, help="consensus rounds: N - 1 realignment rounds after the polish (DESIGN.md section 18)")
    ap.add_argument("--align-links", action="store_true", help="align the links on the newest sequences (DESIGN.md section 26); the result goes to --links-out")
    ap.add_argument("--links-out", default=os.path.join(ROOT, "profiles", "links_probe.json"))
    a = ap.parse_args()
    res = []
    for s in a.sets:
        n, seed, gen = s.split(":")
        res.append(probe(int(n), int(seed), a.repeats, gen == "fast", a.cut_weak, a.polish_rounds, a.align_links))
        print(json.dumps(res[-1]), flush=True)
    with open(a.links_out if a.align_links else a.out, "w") as f:
        json.dump(dict(sets=res), f, indent=1)
        f.write("\n")
