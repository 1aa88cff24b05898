"""Host mirror of the realignment round: placement of every read on its unitig, the banded semi-global DP, the
walk, the votes in unitig coordinates and the consensus, in plain numpy.  Test tooling: nothing here is used by the product.

Who votes.  A read on a unitig (a backbone read; on several vertices, the first vertex counts) and a read with contained == 1 that is
not removed.  Everything is stated in the WHOLE-read frame, so a trim only changes which bases are aligned: the clip [beg, end).

Placement.  A backbone read b at vertex i, orientation o: lead_b = beg (o = 0) or L_b - end (o = 1); its oriented whole read starts at
the raw unitig coordinate x0_b = pos_i - lead_b.  A contained read c takes, among the records whose other read is a backbone read, the
one with the largest span on c (ties: the smallest index).  The record (V = cid forward, H' = rid oriented by the strand; begV on V,
begH on H') gives d = where c's oriented whole read starts in b's FORWARD whole-read frame, and s = c's strand there:

    b = V,  c = H,  strand t:   H'[0] lies at V's position begV - begH           d = begV - begH,               s = t
    b = H,  c = V,  strand 0:   H' = H; V[0] lies at H's position begH - begV    d = begH - begV,               s = 0
    b = H,  c = V,  strand 1:   H' = rc(H); V spans [begH - begV, begH - begV + L_c) of H', which is
                                [L_b - (begH - begV) - L_c, L_b - (begH - begV)) of H, reversed            d = L_b - (begH - begV) - L_c,  s = 1

    hand-checked: L_b = 100, L_c = 40.  V = b, begV = 30, begH = 5, t = 0: c starts at 25 forward.  t = 1: rc(c) starts at 25.
                  H = b, t = 0, begH = 50, begV = 10: c starts at 40.  t = 1, same numbers: V starts at 40 of rc(b), ends at 80, so in
                  b's own direction it is rc(c) on [20, 60): d = 100 - 40 - 40 = 20.

On the unitig: o = 0: x0_c = x0_b + d, orientation s;  o = 1: x0_c = x0_b + (L_b - d - L_c), orientation s ^ 1 (the frame is mirrored
by L_b).  The sequence aligned is the clip in that orientation, n = end - beg bases, starting at x = x0 + lead.

Raw -> current coordinates.  P(x) = ppos_i + (x - pos_i) * pnbases_i // nbases_i for x in segment i (the last i with pos_i <= x),
x itself for x < 0, plen + (x - len) for x >= len.  s = P(x), e = P(x + n).  A read is OUTSIDE when s < -band0/2 or e > plen + band0/2.

Alignment.  Rows i = 0 .. n (bases of the oriented clip), columns q = 0 .. plen (junctions of the unitig), match +1, mismatch -1,
gap -1.  c = s + floor(((e - s) - n) / 2); cell (i, q) exists iff -B/2 <= q - i - c < B/2 and 0 <= q <= plen.  Row 0 is 0.  Rows 1 .. n:
S = max(diagonal + sub, up - 1, left - 1), the direction stored is the first of diagonal, up ('I': a base of the read only), left ('D': a
base of the unitig only) that attains it.  The end is the best cell of row n, ties to the smallest q; the walk goes back to row 0 (up
along q == 0) and has TOUCHED when it visits a cell with p = q - i - c + B/2 <= 0 or >= B - 1 in a row >= 1.  A row n without a cell
that a path reaches counts as touched.  B starts at band0 and doubles while the path touches, up to band_max; a read that touches at
band_max is BAND_CAPPED.  A read with 1000 n_eq < min_identity (n_eq + n_x + n_ins + n_del) is LOW_IDENTITY.  The others vote:
'=' / 'X' base[read base] at q, 'D' del at q, a run of 'I' one ins vote with its first base in the junction before q (q == plen: dropped).
Consensus: pileup_mirror.consensus on every unitig, its own bases the sequence that was aligned against; the new pos of a vertex is
the new offset of its old segment start.

Circles (circular=True, off by default).  A read on a circular unitig is placed on the UNROLLED circle when
place_unrolled admits it: xm = x mod len, s0 = P(xm), e0 = P(xm + n) or plen + P(xm + n - len), e0 >= s0 and max(n, e0 - s0) + band_max
<= plen; s = s0, or s0 + plen when s0 < band_max / 2; status VOTED, pad = 1.  Such a read is aligned against its unitig twice in a row
(2 plen columns), a vote at q goes to row q mod plen, and it is counted as `wrapped` when it votes with e > plen or q_end > plen.  Every
other read is placed, aligned and counted as without the option."""
from __future__ import annotations

import numpy as np

from . import pileup_mirror as P
from .trace_mirror import revcomp, run_lengths
from .unitig_mirror import POLISH_DT

NONE, VOTED, UNPLACED, OUTSIDE, BAND_CAPPED, LOW_IDENTITY = range(6)
NO = 0xFFFFFFFF
PLACE_DT = np.dtype([("unitig", "<u4"), ("orient", "<u4"), ("s", "<i8"), ("e", "<i8"), ("anchor", "<u4"), ("status", "<u4"), ("band", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"),
                     ("n_ins", "<u4"), ("n_del", "<u4"), ("score", "<i4"), ("q_begin", "<i8"), ("q_end", "<i8"), ("op_off", "<u8"), ("nops", "<u4"), ("pad", "<u4")])
COMPARED = ("unitig", "orient", "s", "e", "anchor", "status", "band", "n_eq", "n_x", "n_ins", "n_del", "score", "q_begin", "q_end", "nops")
_NEG = -(1 << 29)
DEFAULTS = dict(band0=512, band_max=4096, min_identity=700, min_depth=3)


def anchor_frame(rec, c: int, Lb: int, Lc: int):
    """(backbone read, d, s) of the contained read c under record rec: see the table above"""
    bV, bH, t = int(rec["begV"]), int(rec["begH"]), int(rec["strand"])
    if int(rec["rid"]) == c and int(rec["cid"]) != c:
        return int(rec["cid"]), bV - bH, t
    if not t:
        return int(rec["rid"]), bH - bV, 0
    return int(rec["rid"]), Lb - (bH - bV) - Lc, 1


def on_unitig(x0b: int, o: int, d: int, s: int, Lb: int, Lc: int):
    """(x0, orientation) of the contained read whose frame on the backbone read is (d, s)"""
    return (x0b + (Lb - d - Lc), s ^ 1) if o else (x0b + d, s)


def lead(beg: int, end: int, L: int, o: int) -> int:
    return L - end if o else beg


def to_current(x: int, pos, nb, cpos, cnb, length: int, plen: int) -> int:
    """P(x) over one unitig's segments (int arrays)"""
    if x < 0:
        return x
    if x >= length:
        return plen + (x - length)
    i = int(np.searchsorted(pos, x, side="right")) - 1
    if not int(nb[i]):
        return int(cpos[i])
    return int(cpos[i]) + (x - int(pos[i])) * int(cnb[i]) // int(nb[i])


def semiglobal_full(read: bytes, unitig: bytes):
    """(score, q_end) of the plain full-matrix semi-global DP: the read global, the unitig window free; ties to the smallest q"""
    x, y = np.frombuffer(read, np.uint8), np.frombuffer(unitig, np.uint8)
    prev = [0] * (len(y) + 1)
    for i in range(1, len(x) + 1):
        cur = [prev[0] - 1] + [0] * len(y)
        for j in range(1, len(y) + 1):
            cur[j] = max(prev[j - 1] + (1 if x[i - 1] == y[j - 1] else -1), prev[j] - 1, cur[j - 1] - 1)
        prev = cur
    best = max(prev)
    return best, prev.index(best)


def semiglobal_banded(read: bytes, unitig: bytes, c: int, B: int):
    """The banded DP and its walk: dict(score, q_begin, q_end, ops (op codes in read order), touch), or dict(touch=True, ops=None) when
    row n has no reachable cell."""
    n, m, half = len(read), len(unitig), B // 2
    rv = np.frombuffer(read, np.uint8)
    upad = np.full(m + 2 * B + 2 * n + 8, 255, np.uint8)             # unitig base j at upad[j + off]
    off = B + n + 4
    p = np.arange(B, dtype=np.int64)
    upad[off:off + m] = np.frombuffer(unitig, np.uint8)
    j0 = c + p - half
    prev = np.where((j0 >= 0) & (j0 <= m), 0, _NEG).astype(np.int64)
    dirs = np.zeros((n + 1, B), np.uint8)
    for i in range(1, n + 1):
        j = j0 + i
        valid = (j >= 0) & (j <= m)
        idx = np.clip(j - 1 + off, 0, len(upad) - 1)
        sub = np.where(upad[idx] == rv[i - 1], 1, -1)
        up = np.concatenate([prev[1:], [_NEG]])
        cd = np.where(valid & (j >= 1), prev + sub, _NEG)
        cu = np.where(valid, up - 1, _NEG)
        s = np.maximum.accumulate(np.maximum(cd, cu) + p) - p
        s[~valid] = _NEG
        dirs[i] = np.where(s == cd, 0, np.where(s == cu, 1, 2))
        prev = s
    best = int(prev.max())
    if best <= _NEG // 2:
        return dict(touch=True, ops=None)
    pe = int(np.argmax(prev))                                         # the first maximum: the smallest q
    i, q = n, int(j0[pe]) + n
    q_end, ops, touch = q, [], False
    while i > 0:
        pp = q - i - c + half
        if pp <= 0 or pp >= B - 1:
            touch = True
            pp = min(max(pp, 0), B - 1)
        d = 1 if q <= 0 else int(dirs[i][pp])
        if d == 0:
            ops.append(0 if unitig[q - 1] == read[i - 1] else 1)
            i, q = i - 1, q - 1
        elif d == 1:
            ops.append(2)
            i -= 1
        else:
            ops.append(3)
            q -= 1
    return dict(score=best, q_begin=q, q_end=q_end, ops=ops[::-1], touch=touch)


def replay(ops, read: bytes, unitig: bytes, q_begin: int, q_end: int):
    """Replays run-length ops against the oriented read and the unitig: the read is consumed whole, the unitig from q_begin to q_end;
    '=' stands on matches and 'X' on mismatches.  Returns dict(n_eq, n_x, n_ins, n_del, score); raises ValueError otherwise."""
    i, q = 0, int(q_begin)
    cnt = [0, 0, 0, 0]
    last = -1
    for w in np.asarray(ops, np.uint32).tolist():
        ln, op = w >> 4, w & 15
        if op > 3 or ln == 0 or op == last:
            raise ValueError("bad run %d%s" % (ln, op))
        last = op
        for _ in range(ln):
            if op <= 1:
                if i >= len(read) or q >= len(unitig) or (read[i] == unitig[q]) != (op == 0):
                    raise ValueError("op %d at read %d, unitig %d" % (op, i, q))
                i, q = i + 1, q + 1
            elif op == 2:
                i += 1
            else:
                q += 1
        cnt[op] += ln
    if i != len(read) or q != int(q_end):
        raise ValueError("ops end at read %d of %d, unitig %d, the record says %d" % (i, len(read), q, q_end))
    return dict(n_eq=cnt[0], n_x=cnt[1], n_ins=cnt[2], n_del=cnt[3], score=cnt[0] - cnt[1] - cnt[2] - cnt[3])


def vote(table, row0: int, plen: int, read: bytes, q_begin: int, op_list, unrolled: bool = False) -> int:
    """adds one read's votes to table[row0 : row0 + plen]; returns how many.  unrolled (section 19): the columns are those of the
    unitig twice in a row, a vote at q goes to row q mod plen, and the read votes at most once per position."""
    rb = P.codes(read)
    i, q, nv, last = 0, int(q_begin), 0, -1
    m = 2 * plen if unrolled else plen
    row = (lambda x: row0 + (x - plen if x >= plen else x)) if unrolled else (lambda x: row0 + x)
    seen = set()
    for op in op_list:
        if op <= 1:
            table[row(q), rb[i]] += 1
            seen.add(row(q))
            nv += 1
            i, q = i + 1, q + 1
        elif op == 2:
            if last != 2 and q < m:
                table[row(q), P.INS + rb[i]] += 1
                nv += 1
            i += 1
        else:
            table[row(q), P.DEL] += 1
            seen.add(row(q))
            nv += 1
            q += 1
        last = op
    assert not unrolled or (q - int(q_begin) <= plen and len(seen) == q - int(q_begin)), "a read on the unrolled circle voted twice for one position"
    return nv


def place_unrolled(x: int, n: int, pos, nb, cpos, cnb, length: int, plen: int, band_max: int):
    """Section 19's rule for one read on a circular unitig: (s, e) on the unrolled circle, or None when the read is not eligible.
    x: the raw coordinate where the clip starts, n: the clip's length; the segment arrays are the unitig's."""
    if plen >= 1 << 29 or length <= 0:
        return None
    xm = x % length                                                   # (Python's %: the floor modulo)
    ym = xm + n
    s0 = to_current(xm, pos, nb, cpos, cnb, length, plen)
    if ym < length:
        e0 = to_current(ym, pos, nb, cpos, cnb, length, plen)
    elif ym - length < length:
        e0 = plen + to_current(ym - length, pos, nb, cpos, cnb, length, plen)
    else:
        return None
    if e0 < s0 or max(n, e0 - s0) + band_max > plen:
        return None
    s = s0 + plen if s0 < band_max // 2 else s0
    return s, s + (e0 - s0)


def place(u, cur, lens, recs, contained, removed, clips=None, band0=512, band_max=4096, circular=False):
    """The placements before any DP: records of PLACE_DT (status VOTED = a candidate) and the counts backbone, contained, unplaced,
    outside, repeated.  clips: None or (beg, end) arrays.  circular (section 19): a read on a circular unitig is placed on the unrolled
    circle when place_unrolled admits it (its pad word is 1); every other read is placed as without the option."""
    nr = len(lens)
    lens = [int(x) for x in lens]
    beg = [0] * nr if clips is None else [int(x) for x in clips[0]]
    end = lens if clips is None else [int(x) for x in clips[1]]
    voff = u["voff"].astype(np.int64).tolist()
    verts, pos, nb = u["verts"].astype(np.int64), u["pos"].astype(np.int64), u["nbases"].astype(np.int64)
    cpos, cnb, coffs = cur["pos"].astype(np.int64), cur["nbases"].astype(np.int64), cur["offsets"].astype(np.int64)
    slot = np.repeat(np.arange(len(voff) - 1), np.diff(voff))
    bvert = {}
    for i, v in enumerate(verts.tolist()):
        bvert.setdefault(v >> 1, i)
    out = np.zeros(nr, PLACE_DT)
    out["unitig"], out["anchor"] = NO, NO
    cnt = dict(backbone=0, contained=0, unplaced=0, outside=0, repeated=len(verts) - len(bvert))
    key = {}
    for x, rec in enumerate(recs):
        for c, b, span in ((int(rec["cid"]), int(rec["rid"]), int(rec["endV"]) - int(rec["begV"])), (int(rec["rid"]), int(rec["cid"]), int(rec["endH"]) - int(rec["begH"]))):
            if contained[c] == 1 and not removed[c] and c not in bvert and b in bvert and (c not in key or span > key[c][0]):
                key[c] = (span, x)
    for r in range(nr):
        L = lens[r]
        if r in bvert:
            i = bvert[r]
            o, k = int(verts[i]) & 1, int(slot[i])
            x0 = int(pos[i]) - lead(beg[r], end[r], L, o)
            cnt["backbone"] += 1
        elif contained[r] == 1 and not removed[r]:
            if r not in key:
                out[r]["status"] = UNPLACED
                cnt["unplaced"] += 1
                continue
            rec = recs[key[r][1]]
            b = int(rec["cid"]) if int(rec["cid"]) != r else int(rec["rid"])
            _, d, s = anchor_frame(rec, r, lens[b], L)
            i = bvert[b]
            ob, k = int(verts[i]) & 1, int(slot[i])
            x0, o = on_unitig(int(pos[i]) - lead(beg[b], end[b], lens[b], ob), ob, d, s, lens[b], L)
            out[r]["anchor"] = key[r][1]
            cnt["contained"] += 1
        else:
            continue
        n = end[r] - beg[r]
        x = x0 + lead(beg[r], end[r], L, o)
        a, z = voff[k], voff[k + 1]
        length, plen = int(u["len"][k]), int(coffs[k + 1] - coffs[k])
        un = place_unrolled(x, n, pos[a:z], nb[a:z], cpos[a:z], cnb[a:z], length, plen, band_max) if circular and int(u["circular"][k]) else None
        if un is not None:
            out[r]["unitig"], out[r]["orient"], out[r]["s"], out[r]["e"], out[r]["status"], out[r]["pad"] = k, o, un[0], un[1], VOTED, 1
            continue
        s_ = to_current(x, pos[a:z], nb[a:z], cpos[a:z], cnb[a:z], length, plen)
        e_ = to_current(x + n, pos[a:z], nb[a:z], cpos[a:z], cnb[a:z], length, plen)
        out[r]["unitig"], out[r]["orient"], out[r]["s"], out[r]["e"] = k, o, s_, e_
        if s_ < -(band0 // 2) or e_ > plen + band0 // 2 or e_ < s_:
            out[r]["status"] = OUTSIDE
            cnt["outside"] += 1
        else:
            out[r]["status"] = VOTED
    return out, cnt


def realign_round(u, cur, seqs, recs, contained, removed, clips=None, band0=512, band_max=4096, min_identity=700, min_depth=3, circular=False):
    """One round: -> dict(offsets, bases, pos, nbases, len, stats of POLISH_DT, placements of PLACE_DT, ops {read: uint32 runs}, table,
    counts).  cur: dict(offsets, bases, pos, nbases) of the sequence to align against (graph_polish_unitigs' result, or a round's).
    circular (section 19): a read that place() put on the unrolled circle is aligned against its unitig twice in a row and votes modulo
    the unitig's length; the counts gain `wrapped`, the voters among them with e > plen or q_end > plen."""
    lens = [len(s) for s in seqs]
    pl, cnt = place(u, cur, lens, recs, contained, removed, clips, band0, band_max, circular)
    coffs = cur["offsets"].astype(np.int64)
    cb = bytes(cur["bases"].tobytes() if hasattr(cur["bases"], "tobytes") else cur["bases"])
    total = int(coffs[-1])
    table = np.zeros((total, P.NCOUNTERS), np.int64)
    ops = {}
    cnt.update(band_capped=0, low_identity=0, voted=0, votes=0, dp_cells=0)
    if circular:
        cnt["wrapped"] = 0
    for r in np.flatnonzero(pl["status"] == VOTED).tolist():
        k, o = int(pl[r]["unitig"]), int(pl[r]["orient"])
        b, e = (0, lens[r]) if clips is None else (int(clips[0][r]), int(clips[1][r]))
        read = seqs[r][b:e]
        if o:
            read = revcomp(read)
        utg = cb[int(coffs[k]):int(coffs[k + 1])]
        plen, unrolled = len(utg), bool(pl[r]["pad"])
        if unrolled:
            utg = utg + utg
        n = len(read)
        c = int(pl[r]["s"]) + ((int(pl[r]["e"]) - int(pl[r]["s"])) - n) // 2
        B = band0
        while True:
            res = semiglobal_banded(read, utg, c, B)
            cnt["dp_cells"] += n * B
            if not res["touch"] or B >= band_max:
                break
            B *= 2
        pl[r]["band"] = B
        if res["ops"] is not None:
            c4 = np.bincount(np.asarray(res["ops"], np.int64), minlength=4)
            pl[r]["n_eq"], pl[r]["n_x"], pl[r]["n_ins"], pl[r]["n_del"] = c4[0], c4[1], c4[2], c4[3]
            pl[r]["score"], pl[r]["q_begin"], pl[r]["q_end"] = res["score"], res["q_begin"], res["q_end"]
        if res["touch"]:
            pl[r]["status"] = BAND_CAPPED
            cnt["band_capped"] += 1
        elif 1000 * int(pl[r]["n_eq"]) < min_identity * (int(pl[r]["n_eq"]) + int(pl[r]["n_x"]) + int(pl[r]["n_ins"]) + int(pl[r]["n_del"])):
            pl[r]["status"] = LOW_IDENTITY
            cnt["low_identity"] += 1
        else:
            cnt["voted"] += 1
            ops[r] = run_lengths(res["ops"])
            pl[r]["nops"] = len(ops[r])
            cnt["votes"] += vote(table, int(coffs[k]), plen, read, res["q_begin"], res["ops"], unrolled)
            if unrolled and (int(pl[r]["e"]) > plen or res["q_end"] > plen):
                cnt["wrapped"] += 1
    # consensus per unitig, and the old segment starts in the new coordinates
    nutg = len(u["len"])
    voff = u["voff"].astype(np.int64).tolist()
    cpos = cur["pos"].astype(np.int64)
    out, offs, npos, nnb, stats = [], [0], [], [], np.zeros(nutg, POLISH_DT)
    for k in range(nutg):
        a, z = int(coffs[k]), int(coffs[k + 1])
        seq, st = P.consensus(cb[a:z], table[a:z], min_depth)
        emitted = emit_counts(cb[a:z], table[a:z], min_depth)
        scan = np.concatenate([[0], np.cumsum(emitted)])
        starts = [int(scan[int(cpos[i])]) for i in range(voff[k], voff[k + 1])]
        npos += starts
        nnb += [y - x for x, y in zip(starts, starts[1:] + [len(seq)])]
        out.append(seq)
        offs.append(offs[-1] + len(seq))
        for f in POLISH_DT.names:
            stats[k][f] = st[f]
    return dict(offsets=np.array(offs, np.uint64), bases=b"".join(out), pos=np.array(npos, np.uint64), nbases=np.array(nnb, np.uint32), len=stats["len_after"].astype(np.uint64),
                stats=stats, placements=pl, ops=ops, table=table.astype(np.uint32), counts=cnt)


def emit_counts(read: bytes, table, min_depth: int):
    """bases that pileup_mirror.consensus emits per position (the junction's base counts with the position behind it)"""
    b = P.codes(read).astype(np.int64)
    n = len(b)
    T = np.asarray(table, np.int64).reshape(n, P.NCOUNTERS)
    depth = T[:, 0:4].sum(1) + T[:, P.DEL]
    c = np.minimum(np.concatenate([[0], depth[:-1]]), depth)
    I = T[:, P.INS:P.INS + 4].sum(1)
    put_ins = (np.arange(n) >= 1) & (c >= min_depth) & (2 * I > c + 1)
    drop = (depth >= min_depth) & (2 * T[:, P.DEL] > depth + 1)
    return put_ins.astype(np.int64) + (~drop).astype(np.int64)
