"""Host mirror of the read correction: the votes of a traced pair, the pileup table, the consensus call and a
global edit distance, in plain numpy.  Test tooling: nothing here is used by the product.  Written from the definition:

The table holds nine counters per base position p of every read: base[4] (votes for A, C, G, T at p), del (votes that the base at p is
not there), ins[4] (votes for ONE base inserted in the junction just before p).  A traced pair (V = read cid, H' = read rid oriented by
the strand, ops in V order from (tbegV, tbegH)) votes on both reads:

    op at (i in V, j in H')   on read V                                   on read H'
    '=' / 'X'                 base[H'[j]] at i                            base[V[i]] at j
    'I' (base of V only)      del at i                                    an inserted base V[i] in the junction before j
    'D' (base of H' only)     an inserted base H'[j] in the junction before i      del at j

and what lands on H' is carried over to H: on strand 1 position j of H' is position lenH - 1 - j of H, junction g' is junction
lenH - g', and a base is complemented.  A run of inserted bases is ONE vote, with the base that comes first in the voted read's own
forward direction.  Junction len has no counters: a vote for it is dropped."""
from __future__ import annotations

import numpy as np

from .trace_mirror import oriented

NCOUNTERS = 9
DEL, INS = 4, 5
_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_ASCII = np.frombuffer(b"ACGT", np.uint8)


def codes(seq: bytes) -> np.ndarray:
    return _CODE[np.frombuffer(seq, np.uint8)]


def votes(ops, trace, seqH: bytes, seqV: bytes, strand: int):
    """Sparse increments of one traced pair: ((posV, ctrV), (posH, ctrH), dropped) -- every entry adds one to counter ctr at position
    pos of the read; positions of H are on H's own forward strand.  `ops` is the whole op array the record's op_off points into.
    dropped = votes that fell on a junction behind a read's last base."""
    w = np.asarray(ops[int(trace["op_off"]):int(trace["op_off"]) + int(trace["nops"])], np.uint32).astype(np.int64)
    ln, op = w >> 4, w & 15
    V, Hp = codes(seqV).astype(np.int64), codes(oriented(seqH, strand)).astype(np.int64)
    lenV, lenH = len(V), len(Hp)
    dv, dh = np.where(op != 3, ln, 0), np.where(op != 2, ln, 0)
    vs, hs = int(trace["tbegV"]) + np.cumsum(dv) - dv, int(trace["tbegH"]) + np.cumsum(dh) - dh       # where every run starts
    pv, cv, ph, ch = [], [], [], []                          # votes on V and on H' (H' frame)

    def expand(sel):
        runs = np.flatnonzero(sel)
        l = ln[runs]
        rep = np.repeat(runs, l)
        return rep, np.arange(int(l.sum())) - np.repeat(np.cumsum(l) - l, l)

    rep, t = expand(op <= 1)                                 # aligned columns: each read votes the other's base
    i, j = vs[rep] + t, hs[rep] + t
    pv.append(i); cv.append(Hp[j])
    ph.append(j); ch.append(V[i])
    rep, t = expand(op == 2)                                 # bases of V only: V votes del, every base
    pv.append(vs[rep] + t); cv.append(np.full(len(rep), DEL))
    rep, t = expand(op == 3)                                 # bases of H' only
    ph.append(hs[rep] + t); ch.append(np.full(len(rep), DEL))
    posV, ctrV = np.concatenate(pv), np.concatenate(cv)
    posHp, ctrHp = np.concatenate(ph), np.concatenate(ch)
    # H' -> H for base and del votes
    if strand:
        posH = lenH - 1 - posHp
        ctrH = np.where(ctrHp < 4, 3 - ctrHp, ctrHp)
    else:
        posH, ctrH = posHp, ctrHp
    # inserted runs, one vote each.  On V: the D runs, junction before the run's i, first base of the run in V's direction = H'[j0]
    dropped = 0
    d = np.flatnonzero(op == 3)
    jn, b = vs[d], Hp[hs[d]]
    keep = jn < lenV
    dropped += int((~keep).sum())
    posV, ctrV = np.concatenate([posV, jn[keep]]), np.concatenate([ctrV, INS + b[keep]])
    # on H: the I runs.  In the frame of H' the junction is the one before the run's j and the run reads V[i0 .. i0 + L); on strand 1 the
    # junction g' of H' is junction lenH - g' of H, and H's forward direction meets the run's LAST base first, complemented
    r = np.flatnonzero(op == 2)
    if strand:
        jn, b = lenH - hs[r], 3 - V[vs[r] + ln[r] - 1]
    else:
        jn, b = hs[r], V[vs[r]]
    keep = jn < lenH
    dropped += int((~keep).sum())
    posH, ctrH = np.concatenate([posH, jn[keep]]), np.concatenate([ctrH, INS + b[keep]])
    return (posV, ctrV), (posH, ctrH), dropped


def pileup(reads, pairs, alns, traces, ops):
    """The table of a read set: (total bases, 9) uint32 in read order, from every record of `traces` with nops > 0.
    reads: list of bytes; pairs / alns / traces: index-aligned record arrays; ops: the op array.  Returns (table, dropped votes)."""
    lens = np.array([len(s) for s in reads], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = []                                                # one index per vote; counted once at the end
    dropped = 0
    for n in np.flatnonzero(traces["nops"] > 0):
        rid, cid, strand = int(pairs[n]["rid"]), int(pairs[n]["cid"]), int(alns[n]["strand"])
        (pV, cV), (pH, cH), d = votes(ops, traces[n], reads[rid], reads[cid], strand)
        assert (pV >= 0).all() and (pV < lens[cid]).all() and (pH >= 0).all() and (pH < lens[rid]).all()
        flat.append((off[cid] + pV) * NCOUNTERS + cV)
        flat.append((off[rid] + pH) * NCOUNTERS + cH)
        dropped += d
    idx = np.concatenate(flat).astype(np.int64) if flat else np.zeros(0, np.int64)
    table = np.bincount(idx, minlength=int(off[-1]) * NCOUNTERS).reshape(int(off[-1]), NCOUNTERS)
    assert table.max(initial=0) < 2 ** 32
    return table.astype(np.uint32), dropped


def consensus(read: bytes, table, min_depth: int = 3):
    """Consensus of one read from ITS rows of the table ((len, 9)).  Returns (bytes, stats dict with the fields of
    bella_consensus_read)."""
    b = codes(read).astype(np.int64)
    n = len(b)
    T = np.asarray(table, np.int64).reshape(n, NCOUNTERS)
    base, dele, ins = T[:, 0:4], T[:, DEL], T[:, INS:INS + 4]
    depth = base.sum(1) + dele
    # junctions: before p, p >= 1
    c = np.minimum(np.concatenate([[0], depth[:-1]]), depth)
    I = ins.sum(1)
    put_ins = (np.arange(n) >= 1) & (c >= min_depth) & (2 * I > c + 1)
    ins_base = np.argmax(ins, 1) if n else np.zeros(0, np.int64)                 # the first maximum = the smallest code
    # positions
    covered = depth >= min_depth
    drop = covered & (2 * dele > depth + 1)
    w = base.copy()
    w[np.arange(n), b] += 1                                  # the read votes once for itself
    mx = w.max(1) if n else np.zeros(0, np.int64)
    call = np.where(w[np.arange(n), b] == mx, b, np.argmax(w, 1) if n else b)
    out_base = np.where(covered, call, b)
    keep = ~drop
    # interleave: junction p, then position p
    slots = np.empty(2 * n, np.int64)
    slots[0::2], slots[1::2] = ins_base, out_base
    use = np.empty(2 * n, bool)
    use[0::2], use[1::2] = put_ins, keep
    seq = _ASCII[slots[use]].tobytes()
    stats = dict(len_before=n, len_after=len(seq), substituted=int((keep & (out_base != b)).sum()), deleted=int(drop.sum()), inserted=int(put_ins.sum()),
                 covered=int(covered.sum()), depth_sum=int(depth.sum()))
    return seq, stats


def edit_distance(a: bytes, b: bytes) -> int:
    """Global (Levenshtein) distance, unit costs.  Row by row; inside a row D[j] = min(cand[j], D[j-1] + 1) is a running minimum of
    cand[j'] - j' (the trick of trace_mirror.extension_optimum's cousin in the row direction)."""
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    m = len(y)
    idx = np.arange(m + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(1, len(x) + 1):
        cand = np.empty(m + 1, np.int64)
        cand[0] = i
        np.minimum(prev[:-1] + (y != x[i - 1]), prev[1:] + 1, out=cand[1:])
        prev = np.minimum.accumulate(cand - idx) + idx
    return int(prev[m])
