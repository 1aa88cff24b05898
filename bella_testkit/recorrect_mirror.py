"""Host mirror of a read correction round: the anchors, the two jobs of every overlap record, section 18's banded
semi-global DP, walk and votes with a corrected read as the target, and the consensus, in plain numpy.  Test tooling: nothing here is
used by the product.

Anchors.  A read of L raw bases has the anchors a[j], j = 0 .. ceil(L / 256): the offset inside its corrected sequence at which raw base
min(256 j, L) was emitted (the emit scan of the consensus), so a[-1] is the corrected length.  P(x), 0 <= x <= L, is realign_mirror's
to_current over the segments pos = 256 j, nb = min(256, L - 256 j), cpos = a[j], cnb = a[j + 1] - a[j].  A later round's new anchor j is
ITS emit scan at the old anchor j.

Jobs.  Record x (V = cid, H = rid, strand t, [begV, endV) on V, [begH, endH) on H' = H oriented by t) gives

    job 2 x      target V   rows H[begH, endH)  (t = 0)  or  rc(H[L_H - endH, L_H - begH))  (t = 1)     raw window on V  [begV, endV)
    job 2 x + 1  target H   rows V[begV, endV)  (t = 0)  or  rc(V[begV, endV))              (t = 1)     raw window on H  [begH, endH) (t = 0),
                                                                                                         [L_H - endH, L_H - begH) (t = 1)

    hand-checked: L_H = 100, t = 1, begH = 10, endH = 70: H' = rc(H), so H'[10, 70) is rc(H[30, 90)); V[begV, endV) reverse-complemented
    lies on H's own strand over [30, 90).

n = the rows, s = P_t(window begin), e = P_t(window end), plen = the target's current length; plen == 0: status NONE.  The alignment, the
band rule, the statuses, the votes and the consensus are realign_mirror's (section 18), the target being the voted side."""
from __future__ import annotations

import numpy as np

from . import pileup_mirror as P
from .realign_mirror import BAND_CAPPED, LOW_IDENTITY, NONE, VOTED, emit_counts, replay, semiglobal_banded, to_current, vote  # noqa: F401
from .trace_mirror import revcomp, run_lengths

STEP = 256
JOB_DT = np.dtype([("record", "<u4"), ("side", "<u4"), ("target", "<u4"), ("query", "<u4"), ("orient", "<u4"), ("status", "<u4"), ("qbeg", "<u4"), ("qend", "<u4"),
                   ("s", "<i8"), ("e", "<i8"), ("band", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4"), ("score", "<i4"), ("q_begin", "<i8"),
                   ("q_end", "<i8"), ("op_off", "<u8"), ("nops", "<u4"), ("pad", "<u4")])
COMPARED = ("record", "side", "target", "query", "orient", "status", "qbeg", "qend", "s", "e", "band", "n_eq", "n_x", "n_ins", "n_del", "score", "q_begin", "q_end", "nops")
CONS_DT = np.dtype([("len_before", "<u4"), ("len_after", "<u4"), ("substituted", "<u4"), ("deleted", "<u4"), ("inserted", "<u4"), ("covered", "<u4"), ("depth_sum", "<u8")])
DEFAULTS = dict(band0=512, band_max=4096, min_identity=700, min_depth=3)


def nanchors(L: int) -> int:
    return (int(L) + STEP - 1) // STEP + 1


def anchors(emitted, old=None):
    """The anchors of one read from the emit counts of the sequence that was decided on (one count per position of it): at the raw
    positions min(256 j, L) when old is None (round 1: the sequence is the raw read), else at the old anchors (a later round)."""
    emitted = np.asarray(emitted, np.int64)
    L = len(emitted)
    scan = np.concatenate([[0], np.cumsum(emitted)]).astype(np.int64)
    at = np.minimum(STEP * np.arange(nanchors(L)), L) if old is None else np.asarray(old, np.int64)
    return scan[at]


def segments(L: int, a):
    """(pos, nb, cpos, cnb) of a read of L raw bases with the anchors a"""
    a = np.asarray(a, np.int64)
    pos = STEP * np.arange(len(a) - 1, dtype=np.int64)
    return pos, np.minimum(STEP, L - pos), a[:-1], np.diff(a)


def to_corrected(x: int, L: int, a, plen: int) -> int:
    pos, nb, cpos, cnb = segments(L, a)
    return to_current(int(x), pos, nb, cpos, cnb, int(L), int(plen))


def jobs(recs, lens):
    """-> (records of JOB_DT with record, side, target, query, orient, qbeg, qend filled in, windows int64[njobs, 2] on the target's raw read)"""
    J = np.zeros(2 * len(recs), JOB_DT)
    W = np.zeros((2 * len(recs), 2), np.int64)
    for x, r in enumerate(recs):
        V, H, t = int(r["cid"]), int(r["rid"]), int(r["strand"])
        bV, eV, bH, eH, LH = int(r["begV"]), int(r["endV"]), int(r["begH"]), int(r["endH"]), int(lens[H])
        onH = (LH - eH, LH - bH) if t else (bH, eH)                   # the H side of the record on H as given
        for side, (tg, q, clip, win) in enumerate(((V, H, onH, (bV, eV)), (H, V, (bV, eV), onH))):
            j = J[2 * x + side]
            j["record"], j["side"], j["target"], j["query"], j["orient"], j["qbeg"], j["qend"] = x, side, tg, q, t, clip[0], clip[1]
            W[2 * x + side] = win
    return J, W


def first_round(seqs, table, min_depth: int = 3):
    """Round 1 = pileup_mirror.consensus of every read from the pileup table: dict(offsets, bases, anchors (one array per read), stats)"""
    lens = [len(s) for s in seqs]
    roff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out, anch, stats = [], [], np.zeros(len(seqs), CONS_DT)
    for r, s in enumerate(seqs):
        rows = table[roff[r]:roff[r + 1]]
        seq, st = P.consensus(s, rows, min_depth)
        anch.append(anchors(emit_counts(s, rows, min_depth)))
        assert int(anch[-1][-1]) == len(seq)
        out.append(seq)
        for f in CONS_DT.names:
            stats[r][f] = st[f]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.uint64)
    return dict(offsets=offs, bases=b"".join(out), anchors=anch, stats=stats)


def flat_anchors(anch):
    """(offsets uint64[nreads + 1], anchors uint64): the per-read lists as the device keeps them"""
    offs = np.concatenate([[0], np.cumsum([len(a) for a in anch])]).astype(np.uint64)
    return offs, (np.concatenate(anch) if anch else np.zeros(0)).astype(np.uint64)


def recorrect_round(cur, seqs, recs, band0=512, band_max=4096, min_identity=700, min_depth=3):
    """One round on `cur` (first_round's dict, or a round's): -> dict(jobs of JOB_DT, ops {job: uint32 runs}, table, offsets, bases, stats of
    CONS_DT relative to cur, anchors, counts)."""
    lens = [len(s) for s in seqs]
    coffs = np.asarray(cur["offsets"]).astype(np.int64)
    cb = bytes(cur["bases"].tobytes() if hasattr(cur["bases"], "tobytes") else cur["bases"])
    total = int(coffs[-1])
    J, W = jobs(recs, lens)
    table = np.zeros((total, P.NCOUNTERS), np.int64)
    ops = {}
    cnt = dict(jobs=len(J), none=0, band_capped=0, low_identity=0, voted=0, votes=0, dp_cells=0)
    for x in range(len(J)):
        j = J[x]
        tg, q = int(j["target"]), int(j["query"])
        plen = int(coffs[tg + 1] - coffs[tg])
        j["s"] = to_corrected(W[x][0], lens[tg], cur["anchors"][tg], plen)
        j["e"] = to_corrected(W[x][1], lens[tg], cur["anchors"][tg], plen)
        read = seqs[q][int(j["qbeg"]):int(j["qend"])]
        if int(j["orient"]):
            read = revcomp(read)
        n = len(read)
        if plen == 0 or n == 0:
            j["status"] = NONE
            cnt["none"] += 1
            continue
        tseq = cb[int(coffs[tg]):int(coffs[tg + 1])]
        c = int(j["s"]) + ((int(j["e"]) - int(j["s"])) - n) // 2
        B = band0
        while True:
            res = semiglobal_banded(read, tseq, c, B)
            cnt["dp_cells"] += n * B
            if not res["touch"] or B >= band_max:
                break
            B *= 2
        j["band"] = B
        if res["ops"] is not None:
            c4 = np.bincount(np.asarray(res["ops"], np.int64), minlength=4)
            j["n_eq"], j["n_x"], j["n_ins"], j["n_del"] = c4[0], c4[1], c4[2], c4[3]
            j["score"], j["q_begin"], j["q_end"] = res["score"], res["q_begin"], res["q_end"]
        if res["touch"]:
            j["status"] = BAND_CAPPED
            cnt["band_capped"] += 1
        elif 1000 * int(j["n_eq"]) < min_identity * (int(j["n_eq"]) + int(j["n_x"]) + int(j["n_ins"]) + int(j["n_del"])):
            j["status"] = LOW_IDENTITY
            cnt["low_identity"] += 1
        else:
            j["status"] = VOTED
            cnt["voted"] += 1
            ops[x] = run_lengths(res["ops"])
            j["nops"] = len(ops[x])
            cnt["votes"] += vote(table, int(coffs[tg]), plen, read, res["q_begin"], res["ops"])
    out, anch, stats = [], [], np.zeros(len(seqs), CONS_DT)
    for r in range(len(seqs)):
        a, z = int(coffs[r]), int(coffs[r + 1])
        seq, st = P.consensus(cb[a:z], table[a:z], min_depth)
        anch.append(anchors(emit_counts(cb[a:z], table[a:z], min_depth), cur["anchors"][r]))
        assert int(anch[-1][-1]) == len(seq)
        out.append(seq)
        for f in CONS_DT.names:
            stats[r][f] = st[f]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.uint64)
    return dict(jobs=J, ops=ops, table=table.astype(np.uint32), offsets=offs, bases=b"".join(out), stats=stats, anchors=anch, counts=cnt)
