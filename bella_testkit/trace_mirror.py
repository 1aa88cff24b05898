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
Ops: 0 '=' 1 'X' (one base of each), 2 'I' (a base of V only), 3 'D' (a base of H' only).

Band.  On B diagonals only the cells with p = j - i + B/2 in [0, B) exist (everything else is minus infinity), rows 0 .. min(n, m + B/2).
Every cell stores the FIRST of diagonal, up ('I'), left ('D') that attains its score; the walk from the best cell back to (0, 0)
follows them (up along j == 0, left along i == 0), and a side whose walk visits p <= 0 or p >= B - 1 (the anchor excluded) has touched.
banded_extension() is that definition for any even B; trace_expect_banded() is the pair-level rule with its widening, op for op."""
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


TOUCH_LOW, TOUCH_HIGH = 1, 2           # which edge a walk visited: p <= 0 (the path drifted towards V), p >= B - 1 (towards H')
_NEGB = -(1 << 29)                     # minus infinity of the banded DP: no sum of it with a column or a step reaches a real score


def banded_extension(h: bytes, v: bytes, B: int):
    """The extension on a band of B diagonals (B even, >= 2): (score, (i, j), ops, touch).  ops: one op code per step of the walk, the
    far end first; touch: 0, or TOUCH_LOW | TOUCH_HIGH for the edges the walk visited (truthy when the side has touched).
    Row by row over the columns of the band: with a linear gap S[i][j] = max_{j' <= j}(cand[j'] + j') - j, cand = max(diagonal, up)."""
    if B < 2 or B & 1:
        raise ValueError("the band must be even and >= 2")
    n, m, half = len(v), len(h), B // 2
    rows = min(n, m + half)
    hv = np.frombuffer(h, np.uint8)
    sub = {b: np.where(hv == b, 1, -1).astype(np.int32) for b in set(v[:rows])}
    J = np.arange(m + 1, dtype=np.int32)
    prev = np.full(m + 1, _NEGB, np.int32)          # S[i - 1][j]; minus infinity where row i - 1 has no cell
    top = min(m, half - 1)
    prev[:top + 1] = -J[:top + 1]
    best, bi, bj = 0, 0, 0
    dirs = [None]                                   # dirs[i] = (first column of row i, its directions)
    for i in range(1, rows + 1):
        lo, hi = max(0, i - half), min(m, i + half - 1)
        a = max(lo, 1)
        cu = prev[lo:hi + 1] - 1                    # (i - 1, j): one diagonal higher, absent for the band's last diagonal
        cd = np.full(hi - lo + 1, _NEGB, np.int32)
        cd[a - lo:] = prev[a - 1:hi] + sub[v[i - 1]][a - 1:hi]
        jj = J[lo:hi + 1]
        s = np.maximum.accumulate(np.maximum(cd, cu) + jj) - jj
        dirs.append((lo, np.where(s == cd, 0, np.where(s == cu, 1, 2)).astype(np.uint8)))
        prev[lo:hi + 1] = s
        mx = int(s.max())
        if mx >= best:
            j = lo + int(np.argmax(s))              # first maximum of the row: its smallest i + j
            if mx > best or i + j < bi + bj:        # (rows come in order of i: on equal score and i + j the earlier row stays)
                best, bi, bj = mx, i, j
    ops, touch = [], 0
    i, j = bi, bj
    while i or j:
        p = j - i + half
        if p <= 0:
            touch |= TOUCH_LOW
        if p >= B - 1:
            touch |= TOUCH_HIGH
        d = 2 if i == 0 else 1 if j == 0 else int(dirs[i][1][j - dirs[i][0]])
        if d == 0:
            ops.append(0 if h[j - 1] == v[i - 1] else 1)
            i, j = i - 1, j - 1
        elif d == 1:
            ops.append(2)
            i -= 1
        else:
            ops.append(3)
            j -= 1
    return best, (bi, bj), ops, touch


def trace_cover_band(n: int, m: int) -> int:
    """the smallest band the device has (a power of two >= 256) that holds the whole rectangle: B >= 2 max(n, m + 1)"""
    b = 256
    while b < 2 * max(n, m + 1):
        b <<= 1
    return b


def first_band(band0: int) -> int:
    b0 = 256
    while b0 < max(band0 or 256, 256) and b0 < (1 << 18):
        b0 <<= 1
    return b0


def run_lengths(op_list):
    """op codes -> uint32 words len << 4 | op, adjacent equal ops merged"""
    a = np.asarray(op_list, np.int64)
    if not len(a):
        return np.zeros(0, np.uint32)
    cut = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    ln = np.diff(np.concatenate([cut, [len(a)]]))
    return (ln << 4 | a[cut]).astype(np.uint32)


def trace_expect_banded(seqH: bytes, seqV: bytes, seedH: int, seedV: int, k: int, aln, band0: int, ext=banded_extension):
    """What a trace that starts with band0 must report, complete: (record, ops, steps).  record: dict(score, tbegH, tendH, tbegV,
    tendV, n_eq, n_x, n_ins, n_del, band, widened); ops: uint32 run-length words in V order (left part, seed, right part, merged
    across both seams); steps: per side (left, right) the list of (band, touch) of every DP the pair ran -- a pair one of whose sides
    touched below its covering band runs again as a whole, every such side with its band doubled.
    ext: the side DP (tests pass a memoising wrapper)."""
    Hp = oriented(seqH, int(aln["strand"]))
    sH, (ml, nl), (mr, nr) = rectangles(len(seqH), len(seqV), seedH, seedV, k, aln)
    sV = seedV
    sides = [(Hp[sH - ml:sH][::-1], seqV[sV - nl:sV][::-1]), (Hp[sH + k:sH + k + mr], seqV[sV + k:sV + k + nr])]
    cover = [trace_cover_band(len(v), len(h)) for h, v in sides]
    band = [min(first_band(band0), c) for c in cover]
    steps, widened = ([], []), 0
    while True:
        res = [ext(h, v, b) for (h, v), b in zip(sides, band)]
        again = False
        for sd in range(2):
            steps[sd].append((band[sd], res[sd][3]))
            if res[sd][3] and band[sd] < cover[sd]:
                band[sd] *= 2
                widened += 1
                again = True
        if not again:
            break
    (sl, (il, jl), ol, _), (sr, (ir, jr), orr, _) = res
    seed = [0 if Hp[sH + t] == seqV[sV + t] else 1 for t in range(k)]
    allops = list(ol) + seed + list(orr)[::-1]
    cnt = np.bincount(np.asarray(allops, np.int64), minlength=4)
    rec = dict(score=sl + sr + sum(1 if o == 0 else -1 for o in seed), tbegH=sH - jl, tendH=sH + k + jr, tbegV=sV - il, tendV=sV + k + ir,
               n_eq=int(cnt[0]), n_x=int(cnt[1]), n_ins=int(cnt[2]), n_del=int(cnt[3]), band=max(band), widened=widened)
    return rec, run_lengths(allops), steps


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
