"""Speed of the read correction next to the trace it rides on: writes profiles/pileup_probe.json.

For every read count (default: the bench set of 10k reads, 10 kb, 15 % error): count, assemble, overlap, align, reset the pileup table,
then ONE call that traces the passed pairs and piles them up on the device without staging the runs on the host, then the consensus.
Reported per set: vote_ms (the vote kernel, all batches) next to dp_ms and walk_ms of the same call, counter increments per second,
the consensus time (three passes + the copy of the corrected bases to the host), what the consensus changed, and the table's bytes.
The expectation DESIGN.md section 10 checks: vote_ms below walk_ms.

--correct-rounds N: the traced pairs' records are accumulated, N - 1 correction rounds follow the consensus, and
per round the stats line (jobs by status, the phase times, DP cells, batches, bases) is printed next to the first trace's dp_ms and kept
under "recorrect" in the set's entry.

--normalize-gaps: after the plain call the table is reset and the same pairs are traced and piled up once more
with every gap run at its canonical position; both vote_ms and both sets of vote stats of the one run are printed and kept under
"normalize" (the consensus and the rounds stay the plain call's)."""
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


def probe(nreads, band, min_depth, correct_rounds=1, correct_band=512, normalize_gaps=False):
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
    eng.pileup_reset()
    reset_s = time.time() - t0
    t0 = time.time()
    eng.trace_pairs(pars, band0=band, pileup=True, keep_ops=False)
    wall = time.time() - t0
    st = eng.trace_stats()
    t0 = time.time()
    offs, bases, stats = eng.consensus(min_depth)
    cons_s = time.time() - t0
    norm = None
    if normalize_gaps:
        plain = eng.vote_stats()
        eng.pileup_reset()
        eng.trace_pairs(pars, band0=band, pileup=True, keep_ops=False, normalize=True)
        nst, nvs = eng.trace_stats(), eng.vote_stats()
        _, nbases, nstats = eng.consensus(min_depth)
        norm = dict(plain=plain, normalized=nvs, vote_ms_plain=plain["vote_ms"], vote_ms_normalized=nvs["vote_ms"], walk_ms_normalized=nst.walk_ms,
                    vote_ratio=nvs["vote_ms"] / max(1e-9, plain["vote_ms"]), corrected_bases=int(len(nbases)), substituted=int(nstats["substituted"].sum()),
                    deleted=int(nstats["deleted"].sum()), inserted=int(nstats["inserted"].sum()))
        print("NORMALIZE %d reads: %s" % (nreads, json.dumps(norm)))
        if correct_rounds > 1:                                       # the rounds below start from the plain consensus, as without the option
            eng.pileup_reset()
            eng.trace_pairs(pars, band0=band, pileup=True, keep_ops=False)
            eng.consensus(min_depth)
    rounds = []
    if correct_rounds > 1:
        eng.graph_reset()
        nrec = eng.graph_add_traced()
        for k in range(2, correct_rounds + 1):
            t0 = time.time()
            eng.recorrect(band0=correct_band, min_depth=min_depth)
            rst = dict(eng.recorrect_stats(), records=int(nrec), wall_s_python_with_copy=time.time() - t0, trace_dp_ms=st.dp_ms)
            print("RECORRECT %d reads, round %d: %s" % (nreads, k, json.dumps(rst)))
            rounds.append(rst)
    out = dict(reads=nreads, bases=int(rs.offsets[-1]), pairs=int(npairs), passed=int(npass), traced=int(st.pairs), band0=int(st.band0), batches=int(st.batches),
               table_bytes=int(eng.pileup_bytes()), reset_ms=1e3 * reset_s, dp_ms=st.dp_ms, walk_ms=st.walk_ms, vote_ms=st.vote_ms, total_ms=st.total_ms,
               call_wall_s_python=wall, votes=int(st.votes), votes_per_s=st.votes / max(1e-9, st.vote_ms / 1e3), vote_bytes_per_s=4 * st.votes / max(1e-9, st.vote_ms / 1e3),
               vote_over_walk=st.vote_ms / max(1e-9, st.walk_ms), ops=int(st.ops), ops_host_bytes=int(st.ops_host_bytes), min_depth=min_depth,
               consensus_ms_with_copy=1e3 * cons_s, corrected_bases=int(len(bases)), mean_depth=float(stats["depth_sum"].sum()) / max(1, int(stats["len_before"].sum())),
               covered_share=float(stats["covered"].sum()) / max(1, int(stats["len_before"].sum())), substituted=int(stats["substituted"].sum()),
               deleted=int(stats["deleted"].sum()), inserted=int(stats["inserted"].sum()))
    if rounds:
        out["recorrect"] = rounds
    if norm:
        out["normalize"] = norm
    eng.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, nargs="+", default=[10000])
    ap.add_argument("--band", type=int, default=0)
    ap.add_argument("--min-depth", type=int, default=3)
    ap.add_argument("--correct-rounds", type=int, default=1)
    ap.add_argument("--correct-band", type=int, default=512)
    ap.add_argument("--normalize-gaps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup_probe.json"))
    a = ap.parse_args()
    res = [probe(n, a.band, a.min_depth, a.correct_rounds, a.correct_band, a.normalize_gaps) for n in a.reads]
    for r in res:
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump(dict(sets=res), f, indent=1)
        f.write("\n")
