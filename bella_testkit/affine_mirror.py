"""Host mirror of the affine-gap pair alignment: section 28's alignment with Gotoh's three matrices and scores
the caller chooses, in plain numpy.  Test tooling: nothing here is used by the product.

Everything this file does not mention is align_mirror's (section 28's), word for word: the pairs, the rc flag, the centre diagonal c,
the cells that exist (-B/2 <= q - i - c < B/2 and 0 <= q <= m), the three modes' ends and their tie rules, feasible(), the doubling of
the band, the statuses, the result fields, the run encoding and the order of the runs.

Scoring.  (a, b, o, e): match +a, mismatch -b, a gap of L bases -(o + e L); 1 <= a <= 255, 0 <= b <= 255, 0 <= o <= 255, 1 <= e <= 255.

Matrices.  Three per cell; a cell that does not exist is minus infinity in all three:

    E[i][q] = max(H[i-1][q] - o - e, E[i-1][q] - e)      a gap that consumes Q ('I')
    F[i][q] = max(H[i][q-1] - o - e, F[i][q-1] - e)      a gap that consumes T ('D')
    H[i][q] = max(H[i-1][q-1] + s(i, q), E[i][q], F[i][q])

Row 0.  Global: H[0][0] = 0, H[0][q] = F[0][q] = -(o + e q) for q > 0; semi-global and dovetail: H[0][q] = 0.  E[0][.] is minus infinity
in every mode, F[0][.] outside global.  Column 0 needs no special case: the E recurrence produces it.

Stored per cell, 4 bits.  hsrc (2 bits): the first of diagonal (0), E (1), F (2) that attains H.  closeE (bit 2): H[i][q] - o >= E[i][q].
closeF (bit 3): H[i][q] - o >= F[i][q].  A set close bit says that a gap arriving at this cell from below (closeE) or from the right
(closeF) is opened here, not extended; ties go to opening.

The walk has a state in {H, E, F} and starts in H at the mode's end cell.  In H at (i, q): hsrc 0 emits '=' or 'X' and moves
diagonally, hsrc 1 switches to E without moving, hsrc 2 to F.  In E: emit 'I', i <- i - 1, then H if closeE of the new cell is set, else
E.  In F: emit 'D', q <- q - 1, then H if closeF of the new cell is set, else F.  In row 0 (global only) it emits 'D' leftwards to (0, 0)
and in column 0 with i > 0 'I' upwards, whatever its state.  The clamp into the band and TOUCHED are section 28's: any visited cell with
p <= 0 or p >= B - 1 in a row >= 1, in any state, or an end that nothing reaches.

The rows are computed the way the device computes them: F[i][q] = max over q' < q of (Hc[q'] + e q') - o - e q with Hc = max(diagonal, E)
-- one prefix maximum per row; in every cell a path reaches that is the recurrence's F (a gap that opens out of F pays o twice and never
wins).  What no path reaches is kept at or near _NEG, never read by a walk.

TOO_LARGE: (n + m) max(a, b, o + e) >= 2^27 (every reachable score stays above _NEG / 2), or the pair's direction bytes n B / 2 at the
band it is to run with exceed `budget`."""
from __future__ import annotations

import numpy as np

from . import align_mirror as lm
from .align_mirror import (ALIGNED, BAND_CAPPED, DOVETAIL, GLOBAL, MODES, OP_DEL, OP_EQ, OP_INS, OP_X, PAIR_DT, RES_DT, SEMIGLOBAL, TOO_LARGE, feasible, oriented,  # noqa: F401
                           records_of)
from .trace_mirror import run_lengths

LINEAR = (1, 1, 0, 1)
MAX_SCORE_CELLS = 1 << 27
_NEG = -(1 << 28)


def check_scoring(scoring) -> tuple:
    a, b, o, e = (int(x) for x in scoring)
    if not (1 <= a <= 255 and 0 <= b <= 255 and 0 <= o <= 255 and 1 <= e <= 255):
        raise ValueError("scoring (%d, %d, %d, %d) is out of range" % (a, b, o, e))
    return a, b, o, e


def too_large(n: int, m: int, scoring) -> bool:
    a, b, o, e = scoring
    return (n + m) * max(a, b, o + e) >= MAX_SCORE_CELLS


def banded(Q: bytes, T: bytes, c: int, B: int, mode: int, scoring=LINEAR):
    """One banded affine DP and its walk: dict(score, q_begin, q_end, t_begin, t_end, ops (op codes in the order of Q), touch), or
    dict(touch=True, ops=None) when no path reaches the end."""
    a, b, o, e = check_scoring(scoring)
    n, m, half = len(Q), len(T), B // 2
    qv = np.frombuffer(Q, np.uint8)
    tpad = np.full(m + 2 * B + 2 * n + 2 * abs(c) + 8, 255, np.uint8)  # base j of T at tpad[j + off]
    off = B + n + abs(c) + 4
    p = np.arange(B, dtype=np.int64)
    tpad[off:off + m] = np.frombuffer(T, np.uint8)
    j0 = c + p - half
    in0 = (j0 >= 0) & (j0 <= m)
    row0 = np.where(j0 > 0, -(o + e * j0), 0) if mode == GLOBAL else np.zeros(B, np.int64)
    H = np.where(in0, row0, _NEG).astype(np.int64)
    E = np.full(B, _NEG, np.int64)
    bits = np.zeros((n + 1, B), np.uint8)
    best, i_end = _NEG, 0                                              # dovetail: the best cell of column m so far
    pm = m - c + half
    if mode == DOVETAIL and 0 <= pm < B:
        best, i_end = 0, 0
    for i in range(1, n + 1):
        j = j0 + i
        valid = (j >= 0) & (j <= m)
        idx = np.clip(j - 1 + off, 0, len(tpad) - 1)
        sub = np.where(tpad[idx] == qv[i - 1], a, -b)
        upH = np.concatenate([H[1:], [_NEG]])
        upE = np.concatenate([E[1:], [_NEG]])
        cd = np.where(valid & (j >= 1), H + sub, _NEG)
        En = np.where(valid, np.maximum(np.maximum(upH - o - e, upE - e), _NEG), _NEG)
        Hc = np.maximum(cd, En)
        incl = np.maximum.accumulate(Hc + e * p)
        excl = np.concatenate([[_NEG], incl[:-1]])
        F = np.where(valid, np.maximum(excl - o - e * p, _NEG), _NEG)
        Hn = np.where(valid, np.maximum(Hc, F), _NEG)
        hsrc = np.where(Hn == cd, 0, np.where(Hn == En, 1, 2))
        bits[i] = hsrc | ((Hn - o >= En).astype(np.uint8) << 2) | ((Hn - o >= F).astype(np.uint8) << 3)
        H, E = Hn, En
        pm = m - i - c + half
        if mode == DOVETAIL and 0 <= pm < B and int(H[pm]) > best:
            best, i_end = int(H[pm]), i
    if mode == GLOBAL:
        pe = m - n - c + half
        best, i, q = (int(H[pe]) if 0 <= pe < B else _NEG), n, m
    elif mode == SEMIGLOBAL:
        best = int(H.max())
        i, q = n, int(j0[int(np.argmax(H))]) + n                       # the first maximum: the smallest q
    else:
        i, q = i_end, m
    if best <= _NEG // 2:
        return dict(touch=True, ops=None)
    q_end, t_end, ops, touch, state = i, q, [], False, 0
    while i > 0 or (mode == GLOBAL and q > 0):
        pp = q - i - c + half
        if pp <= 0 or pp >= B - 1:
            touch = touch or i > 0
            pp = min(max(pp, 0), B - 1)
        if i == 0:
            ops.append(OP_DEL)
            q -= 1
            continue
        if q <= 0:
            ops.append(OP_INS)
            i -= 1
            continue
        w = int(bits[i][pp])
        if (state == 1 and w & 4) or (state == 2 and w & 8):           # the gap that arrived here was opened here
            state = 0
        if state == 0:
            state = min(w & 3, 2)
            if state == 0:
                ops.append(OP_EQ if T[q - 1] == Q[i - 1] else OP_X)
                i, q = i - 1, q - 1
                continue
        if state == 1:
            ops.append(OP_INS)
            i -= 1
        else:
            ops.append(OP_DEL)
            q -= 1
    return dict(score=best, q_begin=0, q_end=q_end, t_begin=q, t_end=t_end, ops=ops[::-1], touch=touch)


def align(bases, records, mode="global", band0=512, band_max=4096, budget=None, dp=banded, scoring=LINEAR):
    """bella_hip_align_sequences_affine: -> dict(results of RES_DT, ops uint32, counts).  align_mirror.align with the score bound in the
    place of n + m >= 2^27 and n * B / 2 direction bytes against `budget`."""
    sc = check_scoring(scoring)
    mode = MODES[mode] if isinstance(mode, str) else int(mode)
    recs = np.asarray(records, PAIR_DT)
    res = np.zeros(len(recs), RES_DT)
    runs, cells, repeated = {}, 0, 0
    for k, rec in enumerate(recs):
        n, m, c = int(rec["q_len"]), int(rec["t_len"]), int(rec["centre"])
        R = res[k]
        B, widened = band0, 0
        R["band"] = B
        if too_large(n, m, sc):
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
            if budget is not None and n * (B // 2) > budget:
                out = None
                break
            out = dp(Q, T, c, B, mode, sc)
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


def replay(runs, Q: bytes, T: bytes, rec, scoring=LINEAR):
    """align_mirror.replay under a scoring: every '=' +a, every 'X' -b, every run of 'I' or 'D' of L bases -(o + e L)."""
    a, b, o, e = check_scoring(scoring)
    out = lm.replay(runs, Q, T, rec)
    gaps = sum(1 for w in np.asarray(runs, np.uint32).tolist() if (w & 15) >= OP_INS)
    out["score"] = a * out["n_eq"] - b * out["n_x"] - e * (out["n_ins"] + out["n_del"]) - o * gaps
    return out
