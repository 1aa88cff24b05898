"""Clipped ends in numpy: the definition the device must EQUAL.  Everything is integer.

For one traced pair with runs r = 0 .. n - 1 (len << 4 | op; op 0 '=' 1 'X' 2 'I' 3 'D') and identity = t permille, 1 <= t <= 999:
w_r = len_r (1000 - t) for an '=' run, -len_r t for any other; P_0 = 0, P_{r+1} = P_r + w_r in 64 bits.  The clip is the (a, b),
0 <= a < b <= n, that maximises P_b - P_a; ties go to the smallest b, for that b to the largest a; a maximum that is not positive
empties the pair (nruns = 0).  The runs are never rewritten."""
import numpy as np

from bella_amd import _lib

EQ, X, INS, DEL = 0, 1, 2, 3
DEFAULT_IDENTITY = 650


def weights(words, t):
    w = np.asarray(words, np.uint32).astype(np.int64)
    op, ln = w & 15, w >> 4
    return np.where(op == EQ, ln * (1000 - t), -ln * t)


def segment(words, t):
    """(a, b, P_b - P_a) of the runs, or (0, 0, 0) when no segment is positive"""
    assert 1 <= t <= 999
    n = len(words)
    if n == 0:
        return 0, 0, 0
    P = np.concatenate([[0], np.cumsum(weights(words, t))]).astype(np.int64)
    lo = np.minimum.accumulate(P[:-1])                        # min over a < b of P_a, for b = 1 .. n
    value = P[1:] - lo
    best = int(value.max())
    if best <= 0:
        return 0, 0, 0
    b = int(np.argmax(value)) + 1                             # the first maximum: the smallest b
    a = int(np.flatnonzero(P[:b] == lo[b - 1])[-1])           # the largest a that reaches it
    return a, b, best


def clip_one(words, tbegV, tbegH, t):
    """one pair's CLIP_RES_DT record (a numpy void)"""
    r = np.zeros(1, _lib.CLIP_RES_DT)[0]
    w = np.asarray(words, np.uint32).astype(np.int64)
    a, b, best = segment(w, t)
    r["begV"] = r["endV"] = tbegV
    r["begH"] = r["endH"] = tbegH
    if b == 0:
        return r
    op, ln = w & 15, w >> 4
    r["first_run"], r["nruns"] = a, b - a
    r["begV"] = tbegV + int(ln[:a][op[:a] != DEL].sum())
    r["begH"] = tbegH + int(ln[:a][op[:a] != INS].sum())
    cnt = [int(ln[a:b][op[a:b] == o].sum()) for o in range(4)]
    r["endV"] = int(r["begV"]) + cnt[EQ] + cnt[X] + cnt[INS]
    r["endH"] = int(r["begH"]) + cnt[EQ] + cnt[X] + cnt[DEL]
    r["n_eq"], r["n_x"], r["n_ins"], r["n_del"] = cnt
    r["score"] = cnt[EQ] - cnt[X] - cnt[INS] - cnt[DEL]
    r["clip_score"] = best
    return r


STAT_COUNTS = ("pairs", "clipped", "emptied", "runs_before", "runs_after", "columns_before", "columns_after", "bases_v_removed", "bases_h_removed")


def _count(st, nops, words, res):
    w = np.asarray(words, np.uint32).astype(np.int64)
    op, ln = w & 15, w >> 4
    st["pairs"] += 1
    st["emptied"] += int(res["nruns"] == 0)
    st["clipped"] += int(0 < res["nruns"] < nops)
    st["runs_before"] += nops
    st["runs_after"] += int(res["nruns"])
    st["columns_before"] += int(ln.sum())
    st["columns_after"] += int(res["n_eq"]) + int(res["n_x"]) + int(res["n_ins"]) + int(res["n_del"])
    st["bases_v_removed"] += int(ln[op != DEL].sum()) - (int(res["endV"]) - int(res["begV"]))
    st["bases_h_removed"] += int(ln[op != INS].sum()) - (int(res["endH"]) - int(res["begH"]))


def clip_pairs(pairs, ops, t=DEFAULT_IDENTITY):
    """what Engine.clip_ops returns for VOTE_PAIR_DT pairs: (CLIP_RES_DT[len(pairs)], the counts of bella_clip_stats)"""
    ops = np.asarray(ops, np.uint32)
    out = np.zeros(len(pairs), _lib.CLIP_RES_DT)
    st = dict.fromkeys(STAT_COUNTS, 0)
    for q, p in enumerate(pairs):
        words = ops[int(p["op_off"]):int(p["op_off"]) + int(p["nops"])]
        out[q] = clip_one(words, int(p["tbegV"]), int(p["tbegH"]), t)
        if len(words):
            _count(st, len(words), words, out[q])
    st["identity"] = t
    return out, st


def clip_traces(traces, ops, t=DEFAULT_IDENTITY):
    """the records trace_pairs(clip=t) hands out, from the records and runs of the call without it: (TRACE_DT[npairs], the counts of
    bella_clip_stats).  An emptied pair keeps op_off, band and widened."""
    ops = np.asarray(ops, np.uint32)
    out = traces.copy()
    st = dict.fromkeys(STAT_COUNTS, 0)
    for q in np.flatnonzero(traces["nops"] > 0):
        tr = traces[q]
        words = ops[int(tr["op_off"]):int(tr["op_off"]) + int(tr["nops"])]
        r = clip_one(words, int(tr["tbegV"]), int(tr["tbegH"]), t)
        _count(st, len(words), words, r)
        o = out[q]
        o["op_off"] = int(tr["op_off"]) + int(r["first_run"])
        o["nops"] = r["nruns"]
        for f, g in (("tbegV", "begV"), ("tendV", "endV"), ("tbegH", "begH"), ("tendH", "endH"), ("n_eq", "n_eq"), ("n_x", "n_x"), ("n_ins", "n_ins"),
                     ("n_del", "n_del"), ("score", "score")):
            o[f] = r[g]
    st["identity"] = t
    return out, st


def vote_pairs(pairs, alns, traces):
    """VOTE_PAIR_DT of the passed, traced pairs: what Engine.pileup_vote takes to repeat the votes of a trace_pairs(pileup=True)"""
    m = np.flatnonzero((alns["passed"] == 1) & (traces["nops"] > 0))
    vp = np.zeros(len(m), _lib.VOTE_PAIR_DT)
    vp["rid"], vp["cid"] = pairs["rid"][m], pairs["cid"][m]
    vp["tbegV"], vp["tbegH"], vp["op_off"], vp["nops"] = traces["tbegV"][m], traces["tbegH"][m], traces["op_off"][m], traces["nops"][m]
    vp["strand"] = alns["strand"][m]
    return vp


# ---- the column-level definition, by brute force (the run-level one above must agree: tests/test_clip_cpu.py) -------------------------
def brute_columns(words, t):
    """the maximum-scoring segment over COLUMNS, O(n^2): (first column, end column, value) with the same tie rule (smallest end, then
    largest start), or None when no segment is positive"""
    w = np.asarray(words, np.uint32).astype(np.int64)
    col = np.repeat(np.where((w & 15) == EQ, 1000 - t, -t), w >> 4)
    P = np.concatenate([[0], np.cumsum(col)])
    best = None
    for e in range(1, len(P)):
        for s in range(e):
            v = int(P[e] - P[s])
            if best is None or v > best[2] or (v == best[2] and e == best[1] and s > best[0]):
                best = (s, e, v)
    return best if best is not None and best[2] > 0 else None
