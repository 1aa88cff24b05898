"""A second statement of one Xavier seed extension (xdrop.hpp, oracle/bella_oracle.c, SURVEY B.5 / DESIGN), in numpy, that also says
WHAT HAPPENED in it: on which step the X-drop fired and in which phase, on which step a sequence ended, which steps kept the previous
direction because the band's maximum was not positive, what every rebase saw, and whether an int8 bound was ever hit.  The case
builders of xdrop_cases.py search with it, and tests/test_xdrop_cases_cpu.py holds it against the oracle on every pair.

It is not the oracle's loop: many extensions advance together, one anti-diagonal per turn, as rows of [n, 32] arrays; a row that has
ended stays where it is.  A step's index is the number of steps completed before it -- (hoff - 31) + (voff - 31) -- which is the count
the kernels report as `steps`; step s runs in launch s // 512 of the sliced kernel.

Band: cell e of anti-diagonal d; a1, a2 = the two anti-diagonals before the one being computed (a3).  Codes: bases 0..3, the string
terminator 4, the pad 5 (terminator matches terminator and pad matches pad, as the bytes 0 and -128 do in the reference)."""
from __future__ import annotations

import numpy as np

W = 32            # cells of the band
LW = 31           # the cells that carry values
NINF = -128
MIDDLE = 15
CUTOFF = 102
NUL, PAD = 4, 5
TAIL = 28         # steps of Phase 4

_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def codes_of(s) -> np.ndarray:
    if isinstance(s, np.ndarray):
        return s.astype(np.uint8)
    c = _CODE[np.frombuffer(bytes(s), np.uint8)]
    assert not (c == 255).any()
    return c


def _triangle(h32, v32):
    """Phase 1: the scores of the 33 x 33 upper-left triangle.  -> (largest score, anti-diagonal i + j = 32 as cells 0..30,
    anti-diagonal i + j = 33 as cells 1..31): cell e of the band is row e + 1 of the first and row e of the second."""
    n = h32.shape[0]
    D = np.full((n, 34, 34), -10 ** 6, np.int64)
    D[:, 0, :] = -np.arange(34)
    D[:, :, 0] = -np.arange(34)
    top = np.zeros(n, np.int64)
    for d in range(2, 34):                                     # cells i + j = d, 1 <= i, j: all of one anti-diagonal at once
        i = np.arange(1, d)
        j = d - i
        same = h32[:, i - 1] == v32[:, j - 1]
        val = np.maximum(D[:, i - 1, j - 1] + np.where(same, 1, -1), np.maximum(D[:, i - 1, j], D[:, i, j - 1]) - 1)
        D[:, i, j] = val
        top = np.maximum(top, val.max(1))
    e = np.arange(LW)
    return top, D[:, e + 1, LW - e], D[:, e + 2, LW - e]


def extend_many(hs, vs, X: int):
    """hs[r], vs[r]: the two sequences of extension r as it reads them (codes 0..3 or ACGT bytes), each at least 32 long.
    -> one dict per extension: best, endH, endV (the extension's own offsets) and the trace fields of the module's header."""
    n = len(hs)
    if n == 0:
        return []
    hs = [codes_of(x) for x in hs]
    vs = [codes_of(x) for x in vs]
    hl = np.array([len(x) + 1 for x in hs], np.int64)
    vl = np.array([len(x) + 1 for x in vs], np.int64)
    assert hl.min() > W and vl.min() > W
    QH = np.full((n, int(hl.max()) + 2 * W), PAD, np.int16)
    QV = np.full((n, int(vl.max()) + 2 * W), PAD, np.int16)
    for r in range(n):
        QH[r, :len(hs[r])] = hs[r]; QH[r, len(hs[r])] = NUL
        QV[r, :len(vs[r])] = vs[r]; QV[r, len(vs[r])] = NUL
    out = [dict(ran=True, p1_drop=False, steps=0, drop_step=None, drop_phase=None, p2_end_step=None, p2_end_seq=None, p4_steps=0,
                nonpos_steps=[], flagged=0, rebases=[], hi_clamps=0, lo_clamps=0, moves_h=0, moves_v=0) for _ in range(n)]

    top, d32, d33 = _triangle(QH[:, :W], QV[:, :W])
    adm = d32.max(1)
    S = {
        "id": np.arange(n), "hl": hl, "vl": vl, "QH": QH, "QV": QV,
        "a1": np.concatenate([d32, np.full((n, 1), NINF)], 1).astype(np.int64),
        "a2": np.concatenate([np.full((n, 1), NINF), d33], 1).astype(np.int64),
        "vqh": np.concatenate([QH[:, 1:W], np.full((n, 1), PAD)], 1).astype(np.int64),
        "vqv": np.concatenate([QV[:, LW:0:-1], np.full((n, 1), PAD)], 1).astype(np.int64),
        "hoff": np.full(n, LW, np.int64), "voff": np.full(n, LW, np.int64),
        "endH": np.full(n, LW, np.int64), "endV": np.full(n, LW, np.int64),
        "best": top.copy(), "off": np.zeros(n, np.int64), "maxpos": np.zeros(n, np.int64),
        "first": np.ones(n, bool), "tail": np.zeros(n, bool), "dir": np.zeros(n, np.int64), "it": np.zeros(n, np.int64),
        "live": adm >= top - X,
    }
    for r in np.flatnonzero(~S["live"]):
        out[r]["p1_drop"] = True

    def settle(rows):
        for q in rows:
            o = out[int(S["id"][q])]
            o["best"], o["endH"], o["endV"] = int(S["best"][q]), int(S["endH"][q]), int(S["endV"][q])
            o["moves_h"], o["moves_v"] = int(S["hoff"][q]) - LW, int(S["voff"][q]) - LW
            o["steps"] = o["moves_h"] + o["moves_v"]
    settle(np.flatnonzero(~S["live"]))

    def sat(raw, operand, rows_id):
        """int8 saturation of `raw` (made from `operand`); counts what it changed that was not at the bound already"""
        hi = raw > 127
        lo = (raw < NINF) & (operand != NINF)
        if hi.any() or lo.any():
            for q in np.flatnonzero(hi.any(1) | lo.any(1)):
                out[int(rows_id[q])]["hi_clamps"] += int(hi[q].sum())
                out[int(rows_id[q])]["lo_clamps"] += int(lo[q].sum())
        return np.clip(raw, NINF, 127)

    turn = 0
    while S["live"].any():
        if turn % 32 == 0 and S["live"].mean() < 0.75:         # forget the rows that have ended
            keep = S["live"]
            for key in S:
                S[key] = S[key][keep]
        turn += 1
        live, ids = S["live"], S["id"]
        a1, a2 = S["a1"], S["a2"]
        nstep = S["hoff"] + S["voff"] - 2 * LW
        # ---- the anti-diagonal
        diag = sat(a1 + np.where(S["vqh"] == S["vqv"], 1, -1), a1, ids)
        nb = np.concatenate([a2[:, 1:], np.full((len(a2), 1), NINF)], 1)
        gap = sat(np.maximum(nb, a2) - 1, np.minimum(nb, a2), ids)
        a3 = np.maximum(diag, gap)
        a3[:, LW] = NINF
        peak = a3.max(1)
        curr = peak + S["off"]
        drop = live & (curr < S["best"] - X)
        for q in np.flatnonzero(drop):
            o = out[int(ids[q])]
            o["drop_step"], o["drop_phase"] = int(nstep[q]), 4 if S["tail"][q] else 2
        inph2 = drop & ~S["tail"]                               # Phase 2 leaves the end where the drop found it; Phase 4 does not move it
        S["endH"] = np.where(inph2, S["hoff"], S["endH"])
        S["endV"] = np.where(inph2, S["voff"], S["endV"])
        go = live & ~drop
        # ---- rebase
        reb = go & (peak > CUTOFF)
        if reb.any():
            mn = a3[:, :LW].min(1)
            span = a3[:, :LW].max(1) - mn
            for q in np.flatnonzero(reb):
                out[int(ids[q])]["rebases"].append((int(nstep[q]), int(mn[q]), int(span[q])))
            sub = np.where(reb, mn, 0)[:, None]
            rows = np.flatnonzero(reb)
            a2[rows] = sat(a2[rows] - sub[rows], a2[rows], ids[rows])
            a3[rows] = sat(a3[rows] - sub[rows], a3[rows], ids[rows])
            S["off"] = S["off"] + sub[:, 0]
            nb = np.concatenate([a2[:, 1:], np.full((len(a2), 1), NINF)], 1)
        S["best"] = np.where(go & (curr > S["best"]), curr, S["best"])
        # ---- where to: Phase 2 follows the first largest positive cell, or keeps the direction it had; Phase 4 alternates
        ph2 = go & ~S["tail"]
        ph4 = go & S["tail"]
        pos = a3.argmax(1)
        found = a3.max(1) > 0
        S["maxpos"] = np.where(ph2 & found, pos, S["maxpos"])
        right2 = S["maxpos"] > MIDDLE
        for q in np.flatnonzero(ph2 & ~found):
            o = out[int(ids[q])]
            if S["first"][q]:
                o["flagged"] = 1
            else:
                o["nonpos_steps"].append((int(nstep[q]), "right" if right2[q] else "down"))
        S["first"] = S["first"] & ~ph2
        S["endH"] = np.where(ph2, S["hoff"], S["endH"])
        S["endV"] = np.where(ph2, S["voff"], S["endV"])
        nxt = S["dir"] ^ 1
        right = (ph2 & right2) | (ph4 & (nxt == 0))
        down = go & ~right
        S["dir"] = np.where(ph4, nxt, S["dir"])
        S["it"] = S["it"] + ph4
        ar = np.arange(len(a2))
        newh = S["QH"][ar, S["hoff"]]
        newv = S["QV"][ar, S["voff"]]
        R, Dn = right[:, None], down[:, None]
        vqh_r = np.concatenate([S["vqh"][:, 1:LW], newh[:, None], np.full((len(a2), 1), PAD)], 1)
        vqv_d = np.concatenate([newv[:, None], S["vqv"][:, :LW]], 1)
        a3_d = np.concatenate([np.full((len(a2), 1), NINF), a3[:, :LW]], 1)
        S["vqh"] = np.where(R, vqh_r, S["vqh"])
        S["vqv"] = np.where(Dn, vqv_d, S["vqv"])
        S["a1"] = np.where(R, nb, np.where(Dn, a2, a1))
        S["a2"] = np.where(R, a3, np.where(Dn, a3_d, a2))
        S["hoff"] = S["hoff"] + right
        S["voff"] = S["voff"] + down
        # ---- a sequence has ended: 28 more steps; the 28 are done: the extension is
        ended = ph2 & ((S["hoff"] >= S["hl"]) | (S["voff"] >= S["vl"]))
        for q in np.flatnonzero(ended):
            o = out[int(ids[q])]
            o["p2_end_step"] = int(nstep[q]) + 1
            o["p2_end_seq"] = "H" if S["hoff"][q] >= S["hl"][q] else "V"
        S["dir"] = np.where(ended, (S["hoff"] >= S["hl"]).astype(np.int64), S["dir"])
        S["tail"] = S["tail"] | ended
        done = drop | (ph4 & (S["it"] >= TAIL))
        for q in np.flatnonzero(done):
            out[int(ids[q])]["p4_steps"] = int(S["it"][q])
        settle(np.flatnonzero(done))
        S["live"] = live & ~done
    return out


NOT_RUN = dict(ran=False, p1_drop=False, steps=0, drop_step=None, drop_phase=None, p2_end_step=None, p2_end_seq=None, p4_steps=0,
               nonpos_steps=[], flagged=0, rebases=[], hi_clamps=0, lo_clamps=0, moves_h=0, moves_v=0, best=0, endH=0, endV=0)


def slope(err: float) -> float:
    """the score a base of a true overlap is worth at error rate err: P(both copies right) - P(not)"""
    p = (1.0 - err) * (1.0 - err)
    return p - (1.0 - p)


def align_many(seqs, seeds, k: int, X: int, err: float = 0.15, delta: float = 0.1):
    """seqs: the reads (ACGT bytes); seeds: (rid, cid, i, j) -- the k-mer at i of read rid (H) and at j of read cid (V).
    -> one dict per seed: score, begH, endH, begV, endV, strand, flagged, steps, ov, passed, and the traces `left` and `right`."""
    cs = {}

    def rd(r):
        if r not in cs:
            cs[r] = codes_of(seqs[r])
        return cs[r]
    jobs_h, jobs_v, plan = [], [], []
    for rid, cid, i, j in seeds:
        h, v = rd(rid), rd(cid)
        strand = int(np.array_equal(3 - h[i:i + k][::-1], v[j:j + k]))
        if strand:                                              # H is read as its reverse complement, the seed moves with it
            h, i = 3 - h[::-1], len(h) - i - k
        eh, ev = i + k, j + k
        slot = [None, None]
        if eh >= W and ev >= W:                                 # left: the prefixes, seed included, back to front
            slot[0] = len(jobs_h); jobs_h.append(h[:eh][::-1]); jobs_v.append(v[:ev][::-1])
        if len(h) - eh >= W and len(v) - ev >= W:               # right: what follows the seed
            slot[1] = len(jobs_h); jobs_h.append(h[eh:]); jobs_v.append(v[ev:])
        plan.append((strand, eh, ev, len(h), len(v), slot))
    ext = extend_many(jobs_h, jobs_v, X)
    phi = slope(err)
    res = []
    for strand, eh, ev, lh, lv, (sl, sr) in plan:
        L = ext[sl] if sl is not None else NOT_RUN
        R = ext[sr] if sr is not None else NOT_RUN
        bH, bV, eH, eV = (eh - L["endH"], ev - L["endV"], eh, ev) if L["ran"] else (0, 0, eh, ev)
        if R["ran"]:
            eH, eV = eH + R["endH"], eV + R["endV"]
        else:
            bH, bV = lh, lv                                     # the reference writes the BEGIN where the end was meant
        score = L["best"] + R["best"]
        u16 = lambda x: int(x) & 0xFFFF
        ov = u16(u16(min(bV, bH)) + u16(min(u16(lv) - eV, u16(lh) - eH)) + (u16(eV - bV) + u16(eH - bH)) // 2)
        thr = np.float32((1.0 - delta) * (phi * float(np.float32(ov))))
        res.append(dict(score=score, begH=bH, endH=eH, begV=bV, endV=eV, strand=strand, flagged=L["flagged"] | R["flagged"],
                        steps=L["steps"] + R["steps"], ov=ov, passed=int(np.float32(score) >= thr), left=L, right=R))
    return res


def align(row: bytes, col: bytes, i: int, j: int, X: int = 7, k: int = 17, err: float = 0.15, delta: float = 0.1):
    return align_many([row, col], [(0, 1, i, j)], k, X, err, delta)[0]
