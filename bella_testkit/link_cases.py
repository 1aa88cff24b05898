"""The synthetic layouts the link-alignment tests share.  Test tooling: nothing here is used by the product.

fork_case(): a trunk of 5,000 bases that continues into two unrelated arms.  Reads of 2,000 bases every 1,200 along both paths, strands
alternating; the reads inside the trunk exist once, the others once per arm.  Every read overlaps its two neighbours by 800 bases and
nothing else, so with max_tip_reads = 0 the graph is three unitigs -- the trunk (3 reads, 4,400 bases) and the arms -- and four links:
trunk -> arm a, trunk -> arm b and their twins.
    arms=(4, 1)        arm b is one read of 2,000 bases: fewer than the expected overlap + band_max / 2, so a window is the whole unitig
    order="abt"        the blocks of reads -- t the trunk's, a and b the arms' -- are numbered in this order: the links that are ALIGNED
                       (the lower-indexed of each twin pair) leave the block that comes first
    rev="tb"           the reads of these blocks are numbered against the line: a unitig is emitted from its lower-numbered end, so this
                       chooses the links' signs -- trunk and arm along the line: + +; arm against: + -; trunk against: - +; both: - -
    deleted=D          D bases of the line are missing from arm a's first read inside its overlap with the trunk, 300 bases in, and its
                       records say it begins 8 bases later than its longer part does: the true path starts D + 8 diagonals below the
                       centre -- with D = 120 on the first diagonal of a band of 256, with D = 248 on the first of a band of 512
    forged=True        one more read of random bases and a forged dovetail record from the trunk's last read to it
    forged="A"         ... of 2,000 times A: against random bases no path scores above 0
    trunk_len=4400, gap=1600   the trunk ends with its last read and the arms' first reads begin 400 bases before that: they share 400
                       bases with the trunk and with each other.  For the whole pipeline: with match +1, mismatch -1, gap -1 an X-drop
                       extension runs on through unrelated bases, so two reads that share 1,400 bases and then part look contained
                       in each other; 400 shared bases of 2,000 do not pass the aligner's threshold
    noise=0.03         the arms' reads carry 3 % substitutions and a quarter as many dropped bases (again for the whole pipeline: the
                       records returned are those of the exact reads)
self_case(): twelve reads around a circle and a read of random bases with a forged dovetail record into read 0: read 0 has two
in-edges, so the circle is a LINEAR unitig whose last vertex links to its own first: a link with a == b.
fork_table(): a pileup table in the style of realign_cases.line_table that deletes every 97th position of the trunk's reads and
inserts a C before every 61st of the other reads, so the two sides of a link change length differently."""
from __future__ import annotations

import numpy as np

from . import graph_mirror as G
from . import unitig_mirror as U

GRAPH = dict(min_overlap=200, fuzz=10)
CLEAN = dict(max_tip_reads=0)
TRUNK, STEP, READ = 5000, 1200, 2000


def fork_case(arms=(4, 4), order="tab", rev="", deleted=0, forged=False, seed=26, trunk_len=TRUNK, gap=STEP, noise=0.0):
    """-> (seqs, recs, trunk read ids)"""
    trunk = U.random_genome(trunk_len, seed)
    starts_t = list(range(0, trunk_len - READ + 1, STEP))              # the reads inside the trunk: 0, 1200, 2400
    first_arm = starts_t[-1] + gap
    lines, reads, block = [], [], {"t": list(range(len(starts_t)))}    # reads: (line or None for the trunk, start, length)
    for s in starts_t:
        reads.append((None, s, READ))
    for a, n in enumerate(arms):
        lines.append(trunk + U.random_genome(first_arm + (n - 1) * STEP + READ - trunk_len, seed + 1 + a))
        block["ab"[a]] = list(range(len(reads), len(reads) + n))
        for i in range(n):
            reads.append((a, first_arm + i * STEP, READ))
    ids = [None] * len(reads)
    for name in (n for n in order if n in block):
        for x in (block[name][::-1] if name in rev else block[name]):
            ids[x] = sum(i is not None for i in ids)
    strands = [i & 1 for i in range(len(reads))]
    seqs = [None] * len(reads)
    pretend = {}                                                       # read -> (start, length) as its records have it
    for x, (a, s, n) in enumerate(reads):
        line = lines[a if a is not None else 0]
        seq = line[s:s + n]
        pretend[x] = (s, n)
        if deleted and a == 0 and s == first_arm:
            seq = line[s:s + 300] + line[s + 300 + deleted:s + n]
            pretend[x] = (s + deleted + 8, n - deleted)
        if noise and a is not None:
            seq = _noisy(seq, noise, np.random.default_rng(seed + 100 + x))
        seqs[ids[x]] = U.revcomp(seq) if strands[x] else seq
    recs = set()
    for a in range(len(arms)):
        on = [x for x, r in enumerate(reads) if r[0] in (None, a)]
        t = G.truth_records([pretend[x][0] for x in on], [pretend[x][1] for x in on], [strands[x] for x in on], min_overlap=GRAPH["min_overlap"])
        # truth_records takes V = the smaller LOCAL id: with reversed ids the record is stated from the other read's side
        for r in t:
            v, h = on[int(r["cid"])], on[int(r["rid"])]
            rec = (ids[v], ids[h], int(r["begV"]), int(r["endV"]), int(r["begH"]), int(r["endH"]), int(r["score"]), int(r["strand"]))
            if ids[v] > ids[h]:
                rec = _swapped(rec, len(seqs[ids[v]]), len(seqs[ids[h]]))
            recs.add(rec)
    trunk_ids = [ids[x] for x in range(len(starts_t))]
    if forged:
        last = ids[len(starts_t) - 1]
        z = len(seqs)
        seqs.append(b"A" * READ if forged == "A" else U.random_genome(READ, seed + 9))
        # the trunk's last read, in the direction of the line, overlaps the new read's first 800 bases with its last 800
        if strands[len(starts_t) - 1] == 0:
            recs.add((last, z, READ - 800, READ, 0, 800, 800, 0))
        else:
            recs.add((last, z, 0, 800, READ - 800, READ, 800, 1))
    out = np.array([r + ((0, 0, 0),) for r in sorted(recs)], G.OVL_DT)
    return seqs, out[np.lexsort((out["rid"], out["cid"]))], trunk_ids


def _noisy(seq: bytes, rate: float, rng) -> bytes:
    """substitutions at `rate`, and a quarter as many single bases dropped (the records no longer fit: for inputs of the whole pipeline)"""
    a = np.frombuffer(seq, np.uint8).copy()
    hit = np.flatnonzero(rng.random(len(a)) < rate)
    a[hit] = np.frombuffer(b"ACGT", np.uint8)[(U._CODE[a[hit]] + rng.integers(1, 4, len(hit))) & 3]
    return a[rng.random(len(a)) >= rate / 4].tobytes()


def _swapped(rec, Lv, Lh):
    """the same overlap with V and H exchanged: coordinates on the new V forward and on the new H' oriented like it"""
    v, h, bV, eV, bH, eH, score, strand = rec
    if not strand:
        return (h, v, bH, eH, bV, eV, score, 0)
    return (h, v, Lh - eH, Lh - bH, Lv - eV, Lv - bV, score, 1)


def fork_table(seqs, trunk_ids):
    """(total bases, 9) uint32: every read votes its own bases five times; every 97th position of a trunk read is deleted, every 61st
    position of another read has a C inserted before it"""
    lens = np.array([len(s) for s in seqs], np.int64)
    roff = np.concatenate([[0], np.cumsum(lens)])
    t = np.zeros((int(roff[-1]), 9), np.uint32)
    for r in range(len(seqs)):
        p = np.arange(lens[r])
        own = U._CODE[np.frombuffer(seqs[r], np.uint8)].astype(np.int64)
        g = roff[r] + p
        t[g, own] = 5
        if r in trunk_ids:
            t[g[p % 97 == 50], 4] = 20
        else:
            t[g[p % 61 == 30], 6] = 10
    return t


def self_case(seed=27):
    """-> (seqs, recs): the circle of realign_cases.circle_case and a read of random bases with a forged dovetail record into read 0"""
    _, seqs, strands, recs = U.circle_input(nreads=12, read_len=1500, step=500, seed=seed, fan=2)
    z = len(seqs)
    seqs = list(seqs) + [U.random_genome(1500, seed + 1)]
    # read 0 forward begins where the new read, oriented by the record's strand, ends
    forged = np.array([(0, z, 0, 700, 800, 1500, 700, 0, (0, 0, 0))], G.OVL_DT)
    recs = np.concatenate([recs, forged])
    return seqs, recs[np.lexsort((recs["rid"], recs["cid"]))]
