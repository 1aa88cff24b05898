"""Host mirror of the link alignment: the ends of two linked unitigs aligned against each other, in plain numpy.
Test tooling: nothing here is used by the product.

Notation.  Link k = (a, b, ovl, rec, flags) of the unitigs claims that a suffix of A^ overlaps a prefix of B^.  cur(u) is the newest
sequence of unitig u (the last realignment round's, else the polish's, else the raw bases), P_u its length, len_u the raw length,
C_u section 18's raw -> current map (realign_mirror.to_current; the identity when nothing was polished).  A^ = cur(a), or its
reverse complement when A_MINUS is set; B^ likewise from b and B_MINUS.

Expected overlaps.  o_a = min(ovl, len_a), o_b = min(ovl, len_b);  oa = P_a - C_a(len_a - o_a) when A is plus, C_a(o_a) when minus;
ob = C_b(o_b) when B is plus, P_b - C_b(len_b - o_b) when minus.

    hand-checked, identity map: len_a = P_a = 5000, ovl = 800.  A plus: the last 800 bases, oa = 5000 - 4200 = 800.  A minus: A^ is the
    reverse complement, its last 800 bases are cur(a)'s first 800: oa = C(800) = 800.  With every 100th base deleted from cur(a) (P_a =
    4950): plus, oa = 4950 - C(4200) = 4950 - 4158 = 792; minus, oa = C(800) = 792.

Windows.  S = band_max // 2, fixed per call.  Columns: X, the last m = min(P_a, oa + S) bases of A^.  Rows: Y, the first n = min(P_b,
ob + S) bases of B^.  Centre diagonal c = m - (oa + ob) // 2: the expected path ends in (about ob, m) and begins in (0, m - about oa).

DP.  Section 18's cell rule, scoring (+1 / -1 / -1), recurrence and direction preference: cell (i, q) exists iff -B/2 <= q - i - c < B/2
and 0 <= q <= m; row 0 is 0.  The END differs: the best existing cell of COLUMN m over the rows 0 .. n, ties to the smallest row -- B^
starts at its first base, A^ ends at its last.  The walk goes from (i_end, m) back to row 0 (up along q == 0) and gives q_begin; it has
TOUCHED when it visits a cell with p = q - i - c + B/2 <= 0 or >= B - 1 in a row >= 1, and a column m without a reachable cell counts as
touched.  B starts at band0 and doubles while the path touches, up to band_max.

Status, tested in this order: a == b: SELF (never aligned); touched at band_max: BAND_CAPPED; best score <= 0: EMPTY;
1000 n_eq < min_identity (n_eq + n_x + n_ins + n_del): LOW_IDENTITY; else ALIGNED.  ovl_a = m - q_begin, ovl_b = i_end; 'I' is a base of
B^ only, 'D' a base of A^ only; the runs are in the order of B^ and only ALIGNED links have runs; a link whose column m no path reached
has all-zero results (but its band and status).

Twins.  The twin of (a, sa, b, sb) is (b, not sb, a, not sa) with the same rec.  Link k, not SELF and not yet paired, takes the smallest
later unpaired link that is its twin.  The lower-indexed link of a pair is aligned, the other DERIVED: runs reversed with 'I' and 'D'
swapped, ovl_a / ovl_b swapped, n_ins / n_del swapped, status, band, score, n_eq, n_x the mate's, mate = the other's index on both.

Runs are laid out in the order the device produces them: the aligned links by their last band, then by index; the derived ones behind,
by index."""
from __future__ import annotations

import numpy as np

from .realign_mirror import to_current
from .trace_mirror import revcomp, run_lengths

ALIGNED, EMPTY, BAND_CAPPED, LOW_IDENTITY, SELF = range(5)
NO = 0xFFFFFFFF
A_MINUS, B_MINUS = 1, 2
ALN_DT = np.dtype([("status", "<u4"), ("band", "<u4"), ("score", "<i4"), ("ovl_a", "<u4"), ("ovl_b", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"),
                   ("n_del", "<u4"), ("mate", "<u4"), ("op_off", "<u8"), ("nops", "<u4"), ("derived", "<u4")])
DEFAULTS = dict(band0=512, band_max=4096, min_identity=700)
_NEG = -(1 << 28)
OP_EQ, OP_X, OP_INS, OP_DEL = range(4)


def dovetail_full(x: bytes, y: bytes):
    """(score, i_end, q_begin) of the plain full-matrix dovetail DP: columns x (a suffix of it is aligned), rows y (a prefix of it); row 0
    is 0; the end is the best cell of the last column, ties to the smallest row; the walk prefers diagonal, then up, then left"""
    m, n = len(x), len(y)
    S, D = [[0] * (m + 1)], [[0] * (m + 1)]
    for i in range(1, n + 1):
        up, row, drow, yb = S[i - 1], [S[i - 1][0] - 1] + [0] * m, [1] + [0] * m, y[i - 1]
        for q in range(1, m + 1):
            cd = up[q - 1] + (1 if x[q - 1] == yb else -1)
            cu, cl = up[q] - 1, row[q - 1] - 1
            s = cd if cd >= cu and cd >= cl else (cu if cu >= cl else cl)
            row[q], drow[q] = s, (0 if s == cd else 1 if s == cu else 2)
        S.append(row)
        D.append(drow)
    col = [S[i][m] for i in range(n + 1)]
    best = max(col)
    i_end = col.index(best)                                            # the first maximum: the smallest row
    i, q = i_end, m
    while i > 0:
        d = D[i][q]
        if d == 0:
            i, q = i - 1, q - 1
        elif d == 1:
            i -= 1
        else:
            q -= 1
    return best, i_end, q


def dovetail_banded(x: bytes, y: bytes, c: int, B: int):
    """The banded DP and its walk: dict(score, i_end, q_begin, ops (op codes in the order of y), touch), or dict(touch=True, ops=None)
    when column m has no reachable cell."""
    m, n, half = len(x), len(y), B // 2
    yv = np.frombuffer(y, np.uint8)
    xpad = np.full(m + 2 * B + 2 * n + 2 * abs(c) + 8, 255, np.uint8)  # base j of x at xpad[j + off]
    off = B + n + abs(c) + 4
    p = np.arange(B, dtype=np.int64)
    xpad[off:off + m] = np.frombuffer(x, np.uint8)
    j0 = c + p - half
    prev = np.where((j0 >= 0) & (j0 <= m), 0, _NEG).astype(np.int64)
    dirs = np.zeros((n + 1, B), np.uint8)
    best, i_end = _NEG, 0
    pm = m - c + half                                                  # the position of column m in row 0
    if 0 <= pm < B:
        best, i_end = 0, 0
    for i in range(1, n + 1):
        j = j0 + i
        valid = (j >= 0) & (j <= m)
        idx = np.clip(j - 1 + off, 0, len(xpad) - 1)
        sub = np.where(xpad[idx] == yv[i - 1], 1, -1)
        up = np.concatenate([prev[1:], [_NEG]])
        cd = np.where(valid & (j >= 1), prev + sub, _NEG)
        cu = np.where(valid, up - 1, _NEG)
        s = np.maximum.accumulate(np.maximum(np.maximum(cd, cu), _NEG) + p) - p
        s = np.maximum(s, _NEG)
        s[~valid] = _NEG
        dirs[i] = np.where(s == cd, 0, np.where(s == cu, 1, 2))
        prev = s
        pm = m - i - c + half
        if 0 <= pm < B and int(s[pm]) > best:
            best, i_end = int(s[pm]), i
    if best <= _NEG // 2:
        return dict(touch=True, ops=None)
    i, q = i_end, m
    ops, touch = [], False
    while i > 0:
        pp = q - i - c + half
        if pp <= 0 or pp >= B - 1:
            touch = True
            pp = min(max(pp, 0), B - 1)
        d = 1 if q <= 0 else int(dirs[i][pp])
        if d == 0:
            ops.append(OP_EQ if x[q - 1] == y[i - 1] else OP_X)
            i, q = i - 1, q - 1
        elif d == 1:
            ops.append(OP_INS)
            i -= 1
        else:
            ops.append(OP_DEL)
            q -= 1
    return dict(score=best, i_end=i_end, q_begin=q, ops=ops[::-1], touch=touch)


def twin_key(link, twin: bool = False):
    a, b, f = int(link["a"]), int(link["b"]), int(link["flags"])
    sa, sb = f & A_MINUS, (f & B_MINUS) >> 1
    return (b, sb ^ 1, a, sa ^ 1, int(link["rec"])) if twin else (a, sa, b, sb, int(link["rec"]))


def pair_twins(links):
    """-> (mate, derived): link k, not SELF and not yet paired, takes the smallest later unpaired link that is its twin"""
    n = len(links)
    mate, derived = [NO] * n, [0] * n
    is_self = [int(l["a"]) == int(l["b"]) for l in links]
    for k in range(n):
        if is_self[k] or mate[k] != NO:
            continue
        want = twin_key(links[k], True)
        for t in range(k + 1, n):
            if not is_self[t] and mate[t] == NO and twin_key(links[t]) == want:
                mate[k], mate[t], derived[t] = t, k, 1
                break
    return mate, derived


def _cur(u, cur):
    """the current sequence of every unitig: offsets, bases, pos, nbases (cur = None: the raw unitigs, u must carry offsets and bases)"""
    src = cur if cur is not None else dict(offsets=u["offsets"], bases=u["bases"], pos=u["pos"], nbases=u["nbases"])
    b = src["bases"]
    return (np.asarray(src["offsets"]).astype(np.int64), bytes(b.tobytes() if hasattr(b, "tobytes") else b), np.asarray(src["pos"]).astype(np.int64),
            np.asarray(src["nbases"]).astype(np.int64))


def expected(u, cur, k: int):
    """link k -> (oa, ob, P_a, P_b): the expected overlaps in current coordinates and the current lengths of the two unitigs"""
    coffs, _, cpos, cnb = _cur(u, cur)
    voff, pos, nb = u["voff"].astype(np.int64), u["pos"].astype(np.int64), u["nbases"].astype(np.int64)
    l = u["links"][k]
    a, b, ovl, f = int(l["a"]), int(l["b"]), int(l["ovl"]), int(l["flags"])

    def C(j, x):
        lo, hi = int(voff[j]), int(voff[j + 1])
        return to_current(x, pos[lo:hi], nb[lo:hi], cpos[lo:hi], cnb[lo:hi], int(u["len"][j]), int(coffs[j + 1] - coffs[j]))
    Pa, Pb, la, lb = int(coffs[a + 1] - coffs[a]), int(coffs[b + 1] - coffs[b]), int(u["len"][a]), int(u["len"][b])
    xa, xb = min(ovl, la), min(ovl, lb)
    oa = C(a, xa) if f & A_MINUS else Pa - C(a, la - xa)
    ob = Pb - C(b, lb - xb) if f & B_MINUS else C(b, xb)
    return oa, ob, Pa, Pb


def windows(u, cur, k: int, band_max: int):
    """link k -> dict(oa, ob, m, n, c, X, Y): the expected overlaps, the window sizes, the centre diagonal and the two oriented windows"""
    coffs, cb, _, _ = _cur(u, cur)
    l = u["links"][k]
    a, b, f = int(l["a"]), int(l["b"]), int(l["flags"])
    oa, ob, Pa, Pb = expected(u, cur, k)
    S = band_max // 2
    m, n = min(Pa, oa + S), min(Pb, ob + S)
    A, Bq = cb[int(coffs[a]):int(coffs[a + 1])], cb[int(coffs[b]):int(coffs[b + 1])]
    A = revcomp(A[:m]) if f & A_MINUS else A[len(A) - m:]              # the last m bases of A^
    Bq = revcomp(Bq[len(Bq) - n:]) if f & B_MINUS else Bq[:n]          # the first n bases of B^
    return dict(oa=oa, ob=ob, m=m, n=n, c=m - (oa + ob) // 2, X=A, Y=Bq)


def derive(runs):
    """a twin's runs from its mate's: reversed, 'I' and 'D' swapped"""
    r = np.asarray(runs, np.uint32)[::-1].copy()
    op = r & 15
    return (r & ~np.uint32(15)) | np.where(op == OP_INS, OP_DEL, np.where(op == OP_DEL, OP_INS, op)).astype(np.uint32)


def align_links(u, cur=None, band0=512, band_max=4096, min_identity=700):
    """bella_hip_graph_align_links: -> dict(alns of ALN_DT, ops uint32, expected = oa per link (0 for SELF), counts)"""
    links = u["links"]
    nl = len(links)
    alns = np.zeros(nl, ALN_DT)
    mate, derived = pair_twins(links)
    alns["mate"], alns["derived"] = mate, derived
    expected = np.zeros(nl, np.int64)
    runs, cells = {}, 0
    for k in range(nl):
        if int(links[k]["a"]) == int(links[k]["b"]):
            alns[k]["status"] = SELF
            continue
        w = windows(u, cur, k, band_max)
        expected[k] = w["oa"]
        if derived[k]:
            continue
        B = band0
        while True:
            res = dovetail_banded(w["X"], w["Y"], w["c"], B)
            cells += w["n"] * B
            if not res["touch"] or B >= band_max:
                break
            B *= 2
        A = alns[k]
        A["band"] = B
        if res["ops"] is not None:
            c4 = np.bincount(np.asarray(res["ops"], np.int64), minlength=4)
            A["n_eq"], A["n_x"], A["n_ins"], A["n_del"] = c4[0], c4[1], c4[2], c4[3]
            A["score"], A["ovl_a"], A["ovl_b"] = res["score"], w["m"] - res["q_begin"], res["i_end"]
        tot = int(A["n_eq"]) + int(A["n_x"]) + int(A["n_ins"]) + int(A["n_del"])
        if res["touch"]:
            A["status"] = BAND_CAPPED
        elif int(A["score"]) <= 0:
            A["status"] = EMPTY
        elif 1000 * int(A["n_eq"]) < min_identity * tot:
            A["status"] = LOW_IDENTITY
        else:
            A["status"] = ALIGNED
            runs[k] = run_lengths(res["ops"])
    ops, at = [], 0
    for k in sorted(runs, key=lambda k: (int(alns[k]["band"]), k)):
        alns[k]["op_off"], alns[k]["nops"] = at, len(runs[k])
        ops.append(np.asarray(runs[k], np.uint32))
        at += len(runs[k])
    for k in range(nl):
        if not derived[k]:
            continue
        M, A = alns[mate[k]], alns[k]
        for f in ("status", "band", "score", "n_eq", "n_x"):
            A[f] = M[f]
        A["ovl_a"], A["ovl_b"], A["n_ins"], A["n_del"] = M["ovl_b"], M["ovl_a"], M["n_del"], M["n_ins"]
        if mate[k] in runs:
            r = derive(runs[mate[k]])
            A["op_off"], A["nops"] = at, len(r)
            ops.append(r)
            at += len(r)
    st = alns["status"]
    al = st == ALIGNED
    counts = dict(links=nl, aligned=int(al.sum()), empty=int((st == EMPTY).sum()), band_capped=int((st == BAND_CAPPED).sum()), low_identity=int((st == LOW_IDENTITY).sum()),
                  self=int((st == SELF).sum()), derived=int(sum(derived)), overlap_before=int(expected[al].sum()), overlap_after=int(alns["ovl_a"][al].astype(np.int64).sum()),
                  jobs=int(nl - (st == SELF).sum() - sum(derived)), dp_cells=cells, ops=at)
    return dict(alns=alns, ops=np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, np.uint32), expected=expected, counts=counts)


def replay(runs, X: bytes, Y: bytes, ovl_a: int, ovl_b: int):
    """Replays run-length ops on the oriented windows: they consume exactly the last ovl_a bases of X and the first ovl_b bases of Y; '='
    stands on equal bases and 'X' on different ones.  Returns dict(n_eq, n_x, n_ins, n_del, score); raises ValueError otherwise."""
    q, i = len(X) - int(ovl_a), 0
    if q < 0:
        raise ValueError("ovl_a %d is longer than the window of %d" % (ovl_a, len(X)))
    cnt, last = [0, 0, 0, 0], -1
    for w in np.asarray(runs, np.uint32).tolist():
        ln, op = w >> 4, w & 15
        if op > 3 or ln == 0 or op == last:
            raise ValueError("bad run %d of op %d" % (ln, op))
        last = op
        for _ in range(ln):
            if op <= 1:
                if q >= len(X) or i >= len(Y) or (X[q] == Y[i]) != (op == OP_EQ):
                    raise ValueError("op %d at from %d, to %d" % (op, q, i))
                q, i = q + 1, i + 1
            elif op == OP_INS:
                i += 1
            else:
                q += 1
        cnt[op] += ln
    if q != len(X) or i != int(ovl_b):
        raise ValueError("the runs end at from %d of %d, to %d, the record says %d" % (q, len(X), i, ovl_b))
    return dict(n_eq=cnt[0], n_x=cnt[1], n_ins=cnt[2], n_del=cnt[3], score=cnt[0] - cnt[1] - cnt[2] - cnt[3])


def cigar(runs) -> bytes:
    """M / I / D, '=' and 'X' merged into M"""
    out, run, last = [], 0, None
    for w in np.asarray(runs, np.uint32).tolist():
        ch = b"MMID"[w & 15:(w & 15) + 1]
        if ch != last and run:
            out.append(b"%d%s" % (run, last))
            run = 0
        last, run = ch, run + (w >> 4)
    if run:
        out.append(b"%d%s" % (run, last))
    return b"".join(out)


def link_lines(u, alns, ops) -> list:
    """the L lines bella_hip_write_unitig_gfa_links writes"""
    names = ["utg%06d%s" % (k + 1, "c" if c else "l") for k, c in enumerate(np.asarray(u["circular"]).tolist())]
    out = []
    for l, a in zip(u["links"], alns):
        head = b"L\t%s\t%s\t%s\t%s\t" % (names[int(l["a"])].encode(), b"-" if int(l["flags"]) & A_MINUS else b"+", names[int(l["b"])].encode(),
                                      b"-" if int(l["flags"]) & B_MINUS else b"+")
        if int(a["status"]) == ALIGNED:
            r = ops[int(a["op_off"]):int(a["op_off"]) + int(a["nops"])]
            out.append(head + b"%s\trc:i:%d\tNM:i:%d\tol:i:%d\n" % (cigar(r), int(l["rec"]), int(a["n_x"]) + int(a["n_ins"]) + int(a["n_del"]), int(l["ovl"])))
        else:
            out.append(head + b"%dM\trc:i:%d\n" % (int(l["ovl"]), int(l["rec"])))
    return out
