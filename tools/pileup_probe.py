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
"normalize" (the consensus and the rounds stay the plain call's).

--clip-ends: after the plain call the table is reset and the same pairs are traced, clipped at --clip-identity and
piled up; clip_ms next to walk_ms and vote_ms of both calls, the clip's statistics and what the consensus then changed are kept under
"clip_ends".  Under "clip_ends_sample": 300 reads of 3 kb at 15 % error with 600 to 1,500 random bases on 40 % of the ends; a fixed-seed
sample of 20 interior reads WITHOUT junk of their own (their partners have it); their edit distance to the templates raw, corrected,
and corrected with the clip."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import numpy as np  # noqa: E402
from bella_amd import BellaPars, Engine  # noqa: E402
from bella_testkit import synth  # noqa: E402


def _dist(job):
    from bella_testkit import pileup_mirror as P
    return P.edit_distance(job[0], job[1])


def clip_sample(identity, min_depth, nreads=300, read_len=3000, seed=23, nsample=20):
    """edit distance to the templates of `nsample` junk-free interior reads of a set whose other reads have junk ends: raw, corrected,
    corrected with clip=identity"""
    import multiprocessing as mp
    from bella_testkit import clip_cases as CC
    from bella_testkit import trace_mirror as M
    rs, head, tail, lens = CC.junk_reads(nreads, read_len=read_len, seed=seed)
    G = max(read_len + 1, round(nreads * read_len / 30.0))
    genome = np.random.default_rng(seed).integers(0, 4, size=G, dtype=np.uint8)
    meta = [tuple(int(x) for x in n.split("_")[1:]) for n in rs.names]                   # (start, length, strand)
    clean = [r for r, (s, L, _) in enumerate(meta) if head[r] == 0 and tail[r] == 0 and s >= read_len and s + L <= G - read_len]
    drawn = sorted(np.random.default_rng(33).choice(clean, min(nsample, len(clean)), replace=False).tolist())
    tmpl = {}
    for r in drawn:
        s, L, strand = meta[r]
        t = synth.BASES[genome[s:s + L]].tobytes()
        tmpl[r] = M.revcomp(t) if strand else t
    seqs = rs.seqs()
    eng = Engine(0)
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    npass = eng.align_pairs(pars)
    jobs = [(bytes(seqs[r]), tmpl[r]) for r in drawn]
    ks = None
    for clip in (None, identity):
        eng.pileup_reset()
        eng.trace_pairs(pars, pileup=True, keep_ops=False, clip=clip)
        if clip:
            ks = eng.clip_stats()
        offs, bases, _ = eng.consensus(min_depth)
        raw = bases.tobytes()
        jobs += [(raw[int(offs[r]):int(offs[r + 1])], tmpl[r]) for r in drawn]
    eng.close()
    with mp.get_context("fork").Pool(8) as pool:
        d = pool.map(_dist, jobs, chunksize=1)
    n = len(drawn)
    d_raw, d_plain, d_clip = (int(sum(d[n * k:n * k + n])) for k in range(3))
    tlen = sum(len(t) for t in tmpl.values())
    return dict(reads=nreads, read_len=read_len, seed=seed, reads_with_junk=int(((head > 0) | (tail > 0)).sum()), junk_bases=int(head.sum() + tail.sum()), passed=int(npass),
                sampled=n, template_bases=tlen, min_depth=min_depth, identity=identity, edit_raw=d_raw, edit_corrected=d_plain, edit_corrected_clip_ends=d_clip,
                clip_over_plain=d_clip / max(1, d_plain), clip_stats={k: int(v) for k, v in ks.items() if k not in ("clip_ms", "pad")})


def probe(nreads, band, min_depth, correct_rounds=1, correct_band=512, normalize_gaps=False, clip_identity=None):
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
    clip = None
    if clip_identity:
        eng.pileup_reset()
        eng.trace_pairs(pars, band0=band, pileup=True, keep_ops=False, clip=clip_identity)
        cst, cks, cvs = eng.trace_stats(), eng.clip_stats(), eng.vote_stats()
        _, cbases, cstats = eng.consensus(min_depth)
        clip = dict(identity=clip_identity, clip_ms=cks["clip_ms"], walk_ms=cst.walk_ms, walk_ms_plain=st.walk_ms, dp_ms=cst.dp_ms, vote_ms=cst.vote_ms, vote_ms_plain=st.vote_ms,
                    clip_over_walk=cks["clip_ms"] / max(1e-9, cst.walk_ms), clip_stats={k: int(v) for k, v in cks.items() if k not in ("clip_ms", "pad")},
                    voting_pairs=int(cvs["pairs"]), votes=int(cvs["votes"]), votes_plain=int(st.votes), corrected_bases=int(len(cbases)),
                    substituted=int(cstats["substituted"].sum()), deleted=int(cstats["deleted"].sum()), inserted=int(cstats["inserted"].sum()))
        print("CLIP-ENDS %d reads: %s" % (nreads, json.dumps(clip)))
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
    if clip:
        out["clip_ends"] = clip
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
    ap.add_argument("--clip-ends", action="store_true")
    ap.add_argument("--clip-identity", type=int, default=650)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup_probe.json"))
    a = ap.parse_args()
    res = [probe(n, a.band, a.min_depth, a.correct_rounds, a.correct_band, a.normalize_gaps, a.clip_identity if a.clip_ends else None) for n in a.reads]
    for r in res:
        print(json.dumps(r))
    doc = dict(sets=res)
    if a.clip_ends:
        doc["clip_ends_sample"] = clip_sample(a.clip_identity, a.min_depth)
        print("CLIP-ENDS sample: %s" % json.dumps(doc["clip_ends_sample"]))
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
