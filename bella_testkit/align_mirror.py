"""Host mirror of the pair alignment: caller-supplied pairs of sequences aligned globally, semi-globally or as a
dovetail, in plain numpy.  Test tooling: nothing here is used by the product.

A call takes one array of upper-case ACGT bytes, a list of pairs, a mode, band0 and band_max.  Pair k names a query Q (q_off, q_len =
n >= 1), a target T (t_off, t_len = m >= 1), flags and a centre diagonal c; with flag bit 0 set Q is reverse-complemented before
anything else.  Rows i = 0 .. n are bases of Q, columns q = 0 .. m bases of T.

DP.  realign_mirror.semiglobal_banded's, word for word: match +1, mismatch -1, gap -1; cell (i, q) exists iff -B/2 <= q - i - c < B/2
and 0 <= q <= m; S = max(diagonal + sub, up - 1, left - 1); the direction stored is the first of diagonal, up ('I': a base of Q only),
left ('D': a base of T only) that attains it; the walk clamps its position into the band and has TOUCHED when it visits a cell with
p = q - i - c + B/2 <= 0 or >= B - 1 in a row >= 1, or when no path reaches the end.  The modes differ in row 0, the end and where the
walk stops:

    GLOBAL (0)      row 0 is -q; the end is the cell (n, m); the walk goes back to (0, 0), leftwards along row 0 as 'D'.  An end or a
                    start outside the band counts as touched.
    SEMIGLOBAL (1)  row 0 is 0; the end is the best cell of row n, ties to the smallest q; the walk stops in row 0.
    DOVETAIL (2)    row 0 is 0; the end is the best cell of column m, ties to the smallest row; the walk stops in row 0.

Bands.  B starts at band0 and doubles while the pair is touched, up to band_max.  A band that cannot hold what the mode needs --
global: the start or the end; the others: any cell of the rectangle -- is doubled without a DP (feasible()).

Status.  TOO_LARGE (2): n + m >= 2^27, or n * B / 4 direction bytes at the band the pair is to run with exceed `budget`; band = that
band.  BAND_CAPPED (1): touched at band_max.  Both leave every field but status, band and widened zero.  ALIGNED (0) otherwise:
score; q_begin, q_end = the rows and t_begin, t_end = the columns the alignment spans; the counts; the runs len << 4 | op in the order of
Q, adjacent runs differing.  A dovetail whose best cell is (0, m) is ALIGNED with no runs.  The runs of all pairs lie by the pairs' last
band, then by index."""
from __future__ import annotations

import numpy as np

from .trace_mirror import revcomp, run_lengths

GLOBAL, SEMIGLOBAL, DOVETAIL = range(3)
MODES = {"global": GLOBAL, "semiglobal": SEMIGLOBAL, "dovetail": DOVETAIL}
ALIGNED, BAND_CAPPED, TOO_LARGE = range(3)
PAIR_RC = 1
PAIR_DT = np.dtype([("q_off", "<u8"), ("t_off", "<u8"), ("q_len", "<u4"), ("t_len", "<u4"), ("flags", "<u4"), ("centre", "<i4")])
RES_DT = np.dtype([("status", "<u4"), ("band", "<u4"), ("widened", "<u4"), ("score", "<i4"), ("q_begin", "<u4"), ("q_end", "<u4"), ("t_begin", "<u4"), ("t_end", "<u4"),
                   ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("op_off", "<u8"), ("nops", "<u4"), ("pad", "<u4")])
COMPARED = tuple(f for f in RES_DT.names if f != "pad")
MAX_CELLS = 1 << 27
_NEG = -(1 << 28)
OP_EQ, OP_X, OP_INS, OP_DEL = range(4)


def default_centre(n: int, m: int, overlap=None) -> int:
    """what the Python wrapper supplies: floor((m - n) / 2), or m - overlap for a dovetail with an expected overlap"""
    return m - int(overlap) if overlap is not None else (m - n) // 2


def feasible(mode: int, n: int, m: int, c: int, B: int) -> bool:
    """whether a band of B holds what the mode needs: global, the start (0, 0) and the end (n, m); else any cell of the rectangle"""
    half = B // 2
    if mode == GLOBAL:
        return -half <= 0 - c < half and -half <= (m - n) - c < half
    return c + half > -n and c - half <= m


def banded(Q: bytes, T: bytes, c: int, B: int, mode: int):
    """One banded DP and its walk: dict(score, q_begin, q_end, t_begin, t_end, ops (op codes in the order of Q), touch), or
    dict(touch=True, ops=None) when no path reaches the end."""
    n, m, half = len(Q), len(T), B // 2
    qv = np.frombuffer(Q, np.uint8)
    tpad = np.full(m + 2 * B + 2 * n + 2 * abs(c) + 8, 255, np.uint8)  # base j of T at tpad[j + off]
    off = B + n + abs(c) + 4
    p = np.arange(B, dtype=np.int64)
    tpad[off:off + m] = np.frombuffer(T, np.uint8)
    j0 = c + p - half
    in0 = (j0 >= 0) & (j0 <= m)
    prev = np.where(in0, -j0 if mode == GLOBAL else 0, _NEG).astype(np.int64)
    dirs = np.zeros((n + 1, B), np.uint8)
    best, i_end = _NEG, 0                                              # dovetail: the best cell of column m so far
    pm = m - c + half
    if mode == DOVETAIL and 0 <= pm < B:
        best, i_end = 0, 0
    for i in range(1, n + 1):
        j = j0 + i
        valid = (j >= 0) & (j <= m)
        idx = np.clip(j - 1 + off, 0, len(tpad) - 1)
        sub = np.where(tpad[idx] == qv[i - 1], 1, -1)
        up = np.concatenate([prev[1:], [_NEG]])
        cd = np.where(valid & (j >= 1), prev + sub, _NEG)
        cu = np.where(valid, up - 1, _NEG)
        s = np.maximum.accumulate(np.maximum(np.maximum(cd, cu), _NEG) + p) - p
        s = np.maximum(s, _NEG)
        s[~valid] = _NEG
        dirs[i] = np.where(s == cd, 0, np.where(s == cu, 1, 2))
        prev = s
        pm = m - i - c + half
        if mode == DOVETAIL and 0 <= pm < B and int(s[pm]) > best:
            best, i_end = int(s[pm]), i
    if mode == GLOBAL:
        pe = m - n - c + half
        best, i, q = (int(prev[pe]) if 0 <= pe < B else _NEG), n, m
    elif mode == SEMIGLOBAL:
        best = int(prev.max())
        i, q = n, int(j0[int(np.argmax(prev))]) + n                    # the first maximum: the smallest q
    else:
        i, q = i_end, m
    if best <= _NEG // 2:
        return dict(touch=True, ops=None)
    q_end, t_end, ops, touch = i, q, [], False
    while i > 0 or (mode == GLOBAL and q > 0):
        pp = q - i - c + half
        if pp <= 0 or pp >= B - 1:
            touch = touch or i > 0
            pp = min(max(pp, 0), B - 1)
        d = 2 if i == 0 else 1 if q <= 0 else int(dirs[i][pp])
        if d == 0:
            ops.append(OP_EQ if T[q - 1] == Q[i - 1] else OP_X)
            i, q = i - 1, q - 1
        elif d == 1:
            ops.append(OP_INS)
            i -= 1
        else:
            ops.append(OP_DEL)
            q -= 1
    return dict(score=best, q_begin=0, q_end=q_end, t_begin=q, t_end=t_end, ops=ops[::-1], touch=touch)


def oriented(bases, rec) -> tuple:
    """(Q, T) of one record of PAIR_DT as bytes, Q reverse-complemented when the record says so"""
    b = bases.tobytes() if hasattr(bases, "tobytes") else bytes(bases)
    Q = b[int(rec["q_off"]):int(rec["q_off"]) + int(rec["q_len"])]
    T = b[int(rec["t_off"]):int(rec["t_off"]) + int(rec["t_len"])]
    return (revcomp(Q) if int(rec["flags"]) & PAIR_RC else Q), T


def align(bases, records, mode="global", band0=512, band_max=4096, budget=None, dp=banded):
    """bella_hip_align_sequences: -> dict(results of RES_DT, ops uint32, counts).  budget: the direction bytes of one batch (None: no
    limit); dp: the banded DP (tests pass a memoising wrapper)."""
    mode = MODES[mode] if isinstance(mode, str) else int(mode)
    recs = np.asarray(records, PAIR_DT)
    res = np.zeros(len(recs), RES_DT)
    runs, cells, repeated = {}, 0, 0
    for k, rec in enumerate(recs):
        n, m, c = int(rec["q_len"]), int(rec["t_len"]), int(rec["centre"])
        R = res[k]
        B, widened = band0, 0
        R["band"] = B
        if n + m >= MAX_CELLS:
            R["status"] = TOO_LARGE
            continue
        while not feasible(mode, n, m, c, B) and B < band_max:
            B, widened = B * 2, widened + 1
        R["band"], R["widened"] = B, widened
        if not feasible(mode, n, m, c, B):
            R["status"] = BAND_CAPPED
            continue
        Q, T = oriented(bases, rec)
        while True:
            R["band"], R["widened"] = B, widened
            if budget is not None and n * (B // 4) > budget:
                out = None
                break
            out = dp(Q, T, c, B, mode)
            cells += n * B
            if not out["touch"] or B >= band_max:
                break
            B, widened, repeated = B * 2, widened + 1, repeated + 1
        if out is None:
            R["status"] = TOO_LARGE
        elif out["touch"]:
            R["status"] = BAND_CAPPED
        else:
            c4 = np.bincount(np.asarray(out["ops"], np.int64), minlength=4)
            R["status"], R["score"] = ALIGNED, out["score"]
            R["q_begin"], R["q_end"], R["t_begin"], R["t_end"] = out["q_begin"], out["q_end"], out["t_begin"], out["t_end"]
            R["n_eq"], R["n_x"], R["n_ins"], R["n_del"] = c4[0], c4[1], c4[2], c4[3]
            runs[k] = run_lengths(out["ops"])
    ops, at = [], 0
    for k in sorted(runs, key=lambda k: (int(res[k]["band"]), k)):
        res[k]["op_off"], res[k]["nops"] = at, len(runs[k])
        ops.append(np.asarray(runs[k], np.uint32))
        at += len(runs[k])
    st = res["status"]
    counts = dict(pairs=len(recs), aligned=int((st == ALIGNED).sum()), band_capped=int((st == BAND_CAPPED).sum()), too_large=int((st == TOO_LARGE).sum()),
                  repeated=repeated, dp_cells=cells, ops=at)
    return dict(results=res, ops=np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, np.uint32), counts=counts)


def records_of(seqs, pairs, mode="global", rc=None, centre=None, overlap=None):
    """what Engine.align_sequences builds: (bases uint8, records of PAIR_DT) of (query, target) index pairs over a list of sequences"""
    lens = np.array([len(s) for s in seqs], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)])
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    recs = np.zeros(len(pr), PAIR_DT)
    for k, (a, b) in enumerate(pr.tolist()):
        n, m = int(lens[a]), int(lens[b])
        recs[k]["q_off"], recs[k]["t_off"], recs[k]["q_len"], recs[k]["t_len"] = offs[a], offs[b], n, m
        recs[k]["flags"] = PAIR_RC if rc is not None and bool(np.broadcast_to(np.asarray(rc), len(pr))[k]) else 0
        if centre is not None:
            recs[k]["centre"] = int(np.broadcast_to(np.asarray(centre), len(pr))[k])
        else:
            recs[k]["centre"] = default_centre(n, m, None if overlap is None else np.broadcast_to(np.asarray(overlap), len(pr))[k])
    return np.frombuffer(b"".join(bytes(s) for s in seqs), np.uint8), recs


def replay(runs, Q: bytes, T: bytes, rec):
    """Replays run-length ops on the oriented Q and T: they consume Q[q_begin, q_end) and T[t_begin, t_end) of the result record exactly;
    '=' stands on equal bases and 'X' on different ones.  Returns dict(n_eq, n_x, n_ins, n_del, score); raises ValueError otherwise."""
    i, q = int(rec["q_begin"]), int(rec["t_begin"])
    cnt, last = [0, 0, 0, 0], -1
    for w in np.asarray(runs, np.uint32).tolist():
        ln, op = w >> 4, w & 15
        if op > 3 or ln == 0 or op == last:
            raise ValueError("bad run %d of op %d" % (ln, op))
        last = op
        for _ in range(ln):
            if op <= 1:
                if i >= len(Q) or q >= len(T) or (Q[i] == T[q]) != (op == OP_EQ):
                    raise ValueError("op %d at query %d, target %d" % (op, i, q))
                i, q = i + 1, q + 1
            elif op == OP_INS:
                i += 1
            else:
                q += 1
        cnt[op] += ln
    if i != int(rec["q_end"]) or q != int(rec["t_end"]):
        raise ValueError("the runs end at query %d, target %d, the record says %d, %d" % (i, q, int(rec["q_end"]), int(rec["t_end"])))
    return dict(n_eq=cnt[0], n_x=cnt[1], n_ins=cnt[2], n_del=cnt[3], score=cnt[0] - cnt[1] - cnt[2] - cnt[3])
