"""Host mirror of the traced alignments: the DEFINITION computed over the full rectangle with numpy, and a
checker that replays a run-length op list against the two reads.  Test tooling: nothing here is used by the product.

Definition.  Scoring: match +1, mismatch -1, gap -1 (linear).  For a pair with X-drop alignment `a` (begH, endH, begV, endV, strand),
V = read cid, H' = read rid, reverse-complemented when strand == 1, the seed at (sH, sV) with sH = lenH - seedH - k when strand == 1:
  left  extension: rows = V[sV-1], V[sV-2], ... down to a.begV, columns = H'[sH-1], H'[sH-2], ... down to a.begH
  right extension: rows = V[sV+k ..  a.endV), columns = H'[sH+k .. a.endH)
(a begin point behind the seed -- the reference overwrites both with the reads' lengths when its right extension does not run -- bounds
nothing: the left rectangle then reaches to the reads' starts)
An extension is a DP with S[0][0] = 0, S[i][0] = -i, S[0][j] = -j, S[i][j] = max(S[i-1][j-1] +- 1, S[i-1][j] - 1, S[i][j-1] - 1); it
ends at the cell with the largest S, ties to the smallest i + j, then the smallest i (i counts bases of V, j bases of H').
Ops: 0 '=' 1 'X' (one base of each), 2 'I' (a base of V only), 3 'D' (a base of H' only)."""
from __future__ import annotations

import numpy as np

OPS = "=XID"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
NEG = -(1 << 28)


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def oriented(seqH: bytes, strand: int) -> bytes:
    return revcomp(seqH) if strand else seqH


def extension_optimum(h: bytes, v: bytes):
    """(score, i, j) of the free-end extension over the whole rectangle: rows = v, columns = h.  Anti-diagonal sweep, vectorised."""
    n, m = len(v), len(h)
    if n == 0 or m == 0:
        return 0, 0, 0                      # along an edge every cell is negative: the anchor is the best cell
    hv = np.frombuffer(h, np.uint8)
    vv = np.frombuffer(v, np.uint8)
    p2 = np.full(n + 1, NEG, np.int32)      # anti-diagonal d - 2, indexed by i
    p1 = np.full(n + 1, NEG, np.int32)
    p2[0] = 0                               # d = 0
    p1[0] = -1                              # d = 1: (0, 1) and (1, 0)
    p1[1] = -1
    best, bi, bj = 0, 0, 0
    for d in range(2, n + m + 1):
        lo, hi = max(0, d - m), min(n, d)   # rows of this anti-diagonal
        cur = np.full(n + 1, NEG, np.int32)
        i = np.arange(max(lo, 1), min(hi, d - 1) + 1)          # cells with i >= 1 and j >= 1
        if len(i):
            sub = np.where(vv[i - 1] == hv[d - i - 1], 1, -1).astype(np.int32)
            cur[i] = np.maximum(np.maximum(p2[i - 1] + sub, p1[i - 1] - 1), p1[i] - 1)
        if lo == 0:
            cur[0] = -d                     # (0, d)
        if hi == d:
            cur[d] = -d                     # (d, 0)
        seg = cur[lo:hi + 1]
        a = int(np.argmax(seg))             # first maximum = smallest i on this anti-diagonal
        if int(seg[a]) > best:              # strictly better only: earlier anti-diagonals (smaller i + j) keep ties
            best, bi, bj = int(seg[a]), lo + a, d - lo - a
        p2, p1 = p1, cur
    return best, bi, bj


def rectangles(lenH: int, lenV: int, seedH: int, seedV: int, k: int, aln):
    """(sH, (m_left, n_left), (m_right, n_right)): the seed on H' and the sizes of the two rectangles, clamped to the reads."""
    strand = int(aln["strand"])
    sH = lenH - seedH - k if strand else seedH
    sV = seedV
    cl = lambda x, hi: max(0, min(int(x), hi))
    ml, nl = cl(sH - int(aln["begH"]), sH), cl(sV - int(aln["begV"]), sV)
    if int(aln["begH"]) > sH or int(aln["begV"]) > sV:      # the reference's overwritten begin points (xavier.h:356-360): whole prefixes
        ml, nl = sH, sV
    mr, nr = cl(int(aln["endH"]) - (sH + k), lenH - sH - k), cl(int(aln["endV"]) - (sV + k), lenV - sV - k)
    return sH, (ml, nl), (mr, nr)


def trace_expect(seqH: bytes, seqV: bytes, seedH: int, seedV: int, k: int, aln):
    """What a trace with a covering band must report: dict(score, tbegH, tendH, tbegV, tendV)."""
    Hp = oriented(seqH, int(aln["strand"]))
    sH, (ml, nl), (mr, nr) = rectangles(len(seqH), len(seqV), seedH, seedV, k, aln)
    sV = seedV
    sl, il, jl = extension_optimum(Hp[sH - ml:sH][::-1], seqV[sV - nl:sV][::-1])
    sr, ir, jr = extension_optimum(Hp[sH + k:sH + k + mr], seqV[sV + k:sV + k + nr])
    seed = sum(1 if Hp[sH + t] == seqV[sV + t] else -1 for t in range(k))
    return dict(score=sl + seed + sr, tbegH=sH - jl, tbegV=sV - il, tendH=sH + k + jr, tendV=sV + k + ir)


def unpack_ops(ops):
    return [(int(w) >> 4, int(w) & 15) for w in ops]


def replay(ops, Hp: bytes, V: bytes, tbegH: int, tendH: int, tbegV: int, tendV: int):
    """Replays run-length ops (uint32 len << 4 | op, V order) from (tbegH, tbegV) on the oriented H' and V.  Raises ValueError on:
    an unknown op, an empty run, two adjacent runs with the same op, '=' on a mismatch or 'X' on a match, a run that leaves a read,
    end points that are not (tendH, tendV).  Returns dict(n_eq, n_x, n_ins, n_del, score)."""
    h0, v0 = int(tbegH), int(tbegV)
    if h0 < 0 or v0 < 0:
        raise ValueError("negative start")
    w = np.asarray(ops, np.uint32).astype(np.int64)
    ln, op = w >> 4, w & 15
    if (op > 3).any():
        raise ValueError("run %d: unknown op" % int(np.flatnonzero(op > 3)[0]))
    if (ln == 0).any():
        raise ValueError("run %d: empty" % int(np.flatnonzero(ln == 0)[0]))
    if len(op) > 1 and (op[1:] == op[:-1]).any():
        raise ValueError("run %d: same op as the run before (runs must be merged)" % (int(np.flatnonzero(op[1:] == op[:-1])[0]) + 1))
    dh, dv = np.where(op != 2, ln, 0), np.where(op != 3, ln, 0)
    hs, vs = h0 + np.cumsum(dh) - dh, v0 + np.cumsum(dv) - dv          # where every run starts
    h, v = h0 + int(dh.sum()), v0 + int(dv.sum())
    if h > len(Hp) or v > len(V):
        raise ValueError("the ops leave a read (end at H %d of %d, V %d of %d)" % (h, len(Hp), v, len(V)))
    dg = np.flatnonzero(op <= 1)
    if len(dg):
        l = ln[dg]
        rep = np.repeat(dg, l)
        within = np.arange(int(l.sum())) - np.repeat(np.cumsum(l) - l, l)
        eq = np.frombuffer(Hp, np.uint8)[hs[rep] + within] == np.frombuffer(V, np.uint8)[vs[rep] + within]
        bad = np.flatnonzero(eq != (op[rep] == 0))
        if len(bad):
            r = int(rep[bad[0]])
            raise ValueError("run %d: %s" % (r, "'=' over a mismatch" if op[r] == 0 else "'X' over a match"))
    if (h, v) != (int(tendH), int(tendV)):
        raise ValueError("ops end at H %d V %d, the record says H %d V %d" % (h, v, tendH, tendV))
    cnt = [int(ln[op == q].sum()) for q in range(4)]
    return dict(n_eq=cnt[0], n_x=cnt[1], n_ins=cnt[2], n_del=cnt[3], score=cnt[0] - cnt[1] - cnt[2] - cnt[3])


def check_trace(tr, ops, seqH: bytes, seqV: bytes, strand: int):
    """replay() of one bella_trace record (numpy record of TRACE_DT) + its counters and score against the ops."""
    o = ops[int(tr["op_off"]):int(tr["op_off"]) + int(tr["nops"])]
    got = replay(o, oriented(seqH, strand), seqV, tr["tbegH"], tr["tendH"], tr["tbegV"], tr["tendV"])
    for f in ("n_eq", "n_x", "n_ins", "n_del", "score"):
        if got[f] != int(tr[f]):
            raise ValueError("%s: ops give %d, the record says %d" % (f, got[f], int(tr[f])))
    return got


def cigar(ops, reverse=False):
    r = unpack_ops(ops)
    if reverse:
        r = r[::-1]
    return "".join("%d%s" % (ln, OPS[op]) for ln, op in r)


def parse_cigar(text: str):
    """'12=1X3I' -> uint32 ops"""
    out, num = [], 0
    for ch in text:
        if ch.isdigit():
            num = num * 10 + ord(ch) - 48
        else:
            out.append(num << 4 | OPS.index(ch))
            num = 0
    return np.array(out, np.uint32)
