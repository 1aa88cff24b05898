"""The inputs the circular realignment tests share.  Test tooling: nothing here is used by the product.

gentle_table(seqs, seed): a polish input that leaves the sequence about 5 % wrong and far above min_identity.  Every position votes its
own base 3 times; with probability 0.02 another base ((b + 1) & 3) gets 5, with 0.015 del gets 5, with 0.015 one ins counter gets 4
(pileup_mirror's layout: four bases, del, four ins).

circle_plus(): realign_cases.circle_case() -- 12 error-free reads of 1,500 bases every 500 around a circle of 6,000 -- plus two
contained reads.  The unitig begins with read 0 (on strand 1) and so runs AGAINST the circle's direction from the circle's base 1,500:
that is its origin, and the reads 1 and 2 run across it.
    12  [1200, 2000) of the circle, strand 0, 8 % substitutions: contained in the reads 1 and 2; two candidate anchors of span 800, the
        tie goes to the record with read 1
    13  [1250, 2250) without every fifth base, strand 1, 4 % substitutions: 800 bases, contained in read 2 alone.  Its record is forged: it
        puts the 800 bases on [1450, 2250), right where the alignment starts (the read's end on the circle: the unitig runs the other
        way) and 200 bases off where it ends.  The path drifts one diagonal every four bases, so at band 256 it touches the band's edge
        after about 500 bases and the band doubles; at 512 it fits.  (A record that is 200 off where the alignment STARTS gives a path
        that no band of 256 reaches, and such a path need not touch anything: found with the mirror.)

noisy_circle(): a circle of 6,000 bases, reads of 1,500 at 15 % error and 30 x cut from genome + genome, a backbone chosen from the true
positions and closed into one circular unitig, polished with the existing mirrors from extensions anchored at the true overlap starts:
tests/test_realign_cpu.py's layout built from truth, on a circle."""
from __future__ import annotations

import numpy as np

from . import graph_mirror as G
from . import pileup_mirror as P
from . import realign_cases as RC
from . import trace_mirror as T
from . import unitig_mirror as U

GLEN, READ, STEP = 6000, 1500, 500


def gentle_table(seqs, seed):
    """(total bases, 9) uint32"""
    rng = np.random.default_rng(seed)
    own = np.concatenate([P.codes(s) for s in seqs]).astype(np.int64)
    n = len(own)
    t = np.zeros((n, P.NCOUNTERS), np.uint32)
    at = np.arange(n)
    t[at, own] = 3
    draw = rng.random((n, 3))
    which = rng.integers(0, 4, n)
    sub, dele, ins = draw[:, 0] < 0.02, draw[:, 1] < 0.015, draw[:, 2] < 0.015
    t[at[sub], (own[sub] + 1) & 3] = 5
    t[at[dele], P.DEL] = 5
    t[at[ins], P.INS + which[ins]] = 4
    return t


def circle_truth():
    """(genome, strands) of realign_cases.circle_case(): read r is genome + genome at [500 r, 500 r + 1500), on strand strands[r]"""
    genome, _, strands, _ = U.circle_input(nreads=12, read_len=READ, step=STEP, seed=19, fan=2)
    return genome, strands


def unitig_template(genome: bytes, u, starts, lens, strands, k: int = 0) -> bytes:
    """the circle as unitig k of `u` spells it: rotated to where the unitig's first vertex begins, in the unitig's direction.  starts /
    lens / strands: where every read lies on genome + genome"""
    v = int(u["verts"][int(u["voff"][k])])
    r, o = v >> 1, v & 1
    n = len(genome)
    if not (int(strands[r]) ^ o):
        a = int(starts[r]) % n
        return genome[a:] + genome[:a]
    a = (int(starts[r]) + int(lens[r])) % n                           # the unitig begins with the read's reverse complement
    return T.revcomp(genome[a:] + genome[:a])


def _contained_record(b: int, sb: int, Lb: int, ob: int, c: int, sc: int, Lc: int, oc: int):
    """the record of read c (id above b's), whole inside read b; s*: where the read lies on genome + genome, o*: its strand"""
    begV = sc - sb if not ob else Lb - (sc + Lc - sb)
    return (b, c, begV, begV + Lc, 0, Lc, Lc, ob ^ oc, (0, 0, 0))


def circle_plus(junk: int = 0):
    """-> (seqs, recs): 14 reads and their records.  junk: that many random bases behind read 12, which no record covers (the reads 1
    and 2 are on strand 0, so the records' coordinates stay what they are): a trim clips them."""
    seqs, recs = RC.circle_case()
    genome, strands = circle_truth()
    assert strands[1] == 0 and strands[2] == 0
    dbl = genome + genome
    rng = np.random.default_rng(190)
    seqs = list(seqs)
    seqs.append(RC._mutate(dbl[1200:2000], 0.08, rng) + U.random_genome(junk, 191))
    thin = np.frombuffer(dbl[1250:2250], np.uint8)[np.arange(1000) % 5 != 2].tobytes()
    seqs.append(U.revcomp(RC._mutate(thin, 0.04, rng)))
    extra = [_contained_record(1, 500, READ, int(strands[1]), 12, 1200, 800, 0),
             _contained_record(2, 1000, READ, int(strands[2]), 12, 1200, 800, 0),
             _contained_record(2, 1000, READ, int(strands[2]), 13, 1450, 800, 1)]           # its first base is the circle's 1250, not 1450
    recs = np.concatenate([recs, np.array(extra, G.OVL_DT)])
    return seqs, recs[np.lexsort((recs["rid"], recs["cid"]))]


def noisy(template: bytes, rng, err=0.15, mix=(0.10, 0.60, 0.30)):
    """a read of `template` at the generator's error mix (substitutions, insertions, deletions): (read, cum) with cum[t] = bases of the
    read in front of template base t"""
    out, cum = [], [0]
    p_sub, p_ins, p_del = (err * m for m in mix)
    for ch in template:
        x = rng.random()
        if x >= p_del:
            out.append(b"ACGT"[(b"ACGT".index(ch) + rng.integers(1, 4)) & 3] if x < p_del + p_sub else ch)
            if p_del + p_sub <= x < p_del + p_sub + p_ins:
                out.append(b"ACGT"[rng.integers(0, 4)])
        cum.append(len(out))
    return bytes(out), cum


def circular_reads(glen: int, nreads: int, read_len: int, err: float, seed: int, mix=(0.10, 0.60, 0.30)):
    """`nreads` reads of `read_len` template bases at uniform starts around a random circle of `glen` bases (cut from genome + genome),
    random strands, synth.make_reads' error model and names ("r<i>_<start>_<length>_<strand>"): -> (genome, seqs, names)"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, glen, dtype=np.uint8)
    p_sub, p_ins, p_del = (err * m for m in mix)
    start, strand = rng.integers(0, glen, nreads), rng.integers(0, 2, nreads)
    seqs, names = [], []
    for i in range(nreads):
        t = genome[(int(start[i]) + np.arange(read_len)) % glen]
        if strand[i]:
            t = 3 - t[::-1]
        x = rng.random(read_len)
        base = np.where((x >= p_del) & (x < p_del + p_sub), (t + rng.integers(1, 4, read_len)) & 3, t)
        pair = np.stack([base, rng.integers(0, 4, read_len)], 1)
        use = np.stack([x >= p_del, (x >= p_del + p_sub) & (x < p_del + p_sub + p_ins)], 1)
        seqs.append(P._ASCII[pair[use]].tobytes())
        names.append("r%d_%d_%d_%d" % (i, int(start[i]), read_len, int(strand[i])))
    return P._ASCII[genome].tobytes(), seqs, names


def noisy_circle(seed=77, glen=GLEN, L=READ, cover=30):
    """-> dict(genome, starts, strands, seqs, chain, u, recs, contained, polished)"""
    rng = np.random.default_rng(seed)
    genome = U.random_genome(glen, seed + 1)
    dbl = genome + genome
    n = cover * glen // L
    starts = np.sort(np.concatenate([[0], rng.integers(0, glen, n - 1)]))
    strands = rng.integers(0, 2, n)
    fwd, cums = zip(*(noisy(dbl[s:s + L], rng) for s in starts.tolist()))
    seqs = [T.revcomp(f) if o else f for f, o in zip(fwd, strands.tolist())]
    chain = [0]                                                       # around the circle, every next read the furthest that still shares 500 bases
    while starts[chain[-1]] + L - 500 < glen:
        chain.append(max(r for r in range(n) if starts[r] <= starts[chain[-1]] + L - 500))
    assert len(chain) >= 5 and starts[chain[-1]] < glen
    nxt = chain[1:] + [chain[0]]
    gap = [(int(starts[b]) - int(starts[a])) % glen for a, b in zip(chain, nxt)]
    nb = [cums[a][g] for a, g in zip(chain, gap)]
    u = dict(voff=np.array([0, len(chain)], np.uint64), verts=np.array([2 * r + int(strands[r]) for r in chain], np.uint32),
             pos=np.array(np.concatenate([[0], np.cumsum(nb)[:-1]]), np.uint64), nbases=np.array(nb, np.uint32), len=np.array([sum(nb)], np.uint64),
             circular=np.array([1], np.uint8))
    # every read against every backbone read it shares >= 500 template bases with, on the circle: an extension from the overlap's true start
    pairs, alns, traces, ops, recs = [], [], [], [], []
    for b in chain:
        for x in range(n):
            if x == b or (x in chain and x < b):
                continue
            for turn in (-glen, 0, glen):                             # x as it lies one turn before, on, one turn behind b
                sx = int(starts[x]) + turn
                lo, hi = max(int(starts[b]), sx), min(int(starts[b]), sx) + L
                if hi - lo < 500:
                    continue
                v, h = min(b, x), max(b, x)
                sv, sh = (int(starts[b]), sx) if v == b else (sx, int(starts[b]))
                if strands[v] == 0:
                    tv, th = cums[v][lo - sv], cums[h][lo - sh]
                else:
                    tv, th = len(fwd[v]) - cums[v][hi - sv], len(fwd[h]) - cums[h][hi - sh]
                st = int(strands[v] ^ strands[h])
                Hp = T.oriented(seqs[h], st)
                score, (i, j), o, _ = T.banded_extension(Hp[th:], seqs[v][tv:], 256)
                runs = T.run_lengths(o[::-1])
                pairs.append((h, v)); alns.append(st); traces.append((len(runs), sum(len(q) for q in ops), tv, th))
                ops.append(runs)
                recs.append((v, h, tv, tv + i, th, th + j, score, st, (0, 0, 0)))
                break
    pairs = np.array(pairs, [("rid", "<u4"), ("cid", "<u4")])
    alns = np.array(alns, [("strand", "<u4")])
    traces = np.array(traces, [("nops", "<u4"), ("op_off", "<u8"), ("tbegV", "<i4"), ("tbegH", "<i4")])
    table, _ = P.pileup(seqs, pairs, alns, traces, np.concatenate(ops))
    recs = np.array(recs, G.OVL_DT)
    contained = np.array([0 if r in chain else 1 for r in range(n)], np.uint8)
    return dict(genome=genome, starts=starts, strands=strands, seqs=seqs, chain=chain, u=u, recs=recs, contained=contained, polished=U.polished(u, seqs, table, 3))
