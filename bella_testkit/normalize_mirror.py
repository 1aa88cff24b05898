"""Host mirror of the gap normalisation of the pileup votes, in plain numpy.  Test tooling: nothing here is used
by the product.  The device (k_pile_vote_norm, pileup.hpp) must EQUAL what this file computes.

A traced pair has runs R_0 .. R_{n-1} in V order from (tbegV, tbegH); run k starts at (i_k, j_k).  For a gap run k of length L let
S = V, x = i_k for 'I' and S = H', x = j_k for 'D'.  Two shifts per gap run:

    sL_k: 0 unless k >= 1 and R_{k-1} is an '=' run (length d); else the largest s in [0, d] with S[x-1-t] == S[x+L-1-t] for all t < s
    sR_k: 0 unless k <= n-2 and R_{k+1} is an '=' run (length d'); else the largest s in [0, d'] with S[x+t] == S[x+L+t] for all t < s

(a comparison that would leave S ends the shift: it cannot happen while the runs lie inside both reads).  Every gap run shifts
independently, inside its ORIGINAL neighbouring '=' run only: never across an 'X', another gap or an end of the pair.

The left-normalised alignment A_L: R_{k-1} keeps d - sL_k columns, the gap starts at (i_k - sL_k, j_k - sL_k), sL_k '=' columns follow
it (by the periodicity just tested they are still matches and carry the same base pairs).  A_R is the mirror image with sR.  The votes
are section 10's (pileup_mirror.votes), on V and on H of a strand-0 pair from A_L, on H of a strand-1 pair from A_R: right in V order is
left in H's own forward direction, so every gap votes as far towards the START of the voted read as its '=' neighbour lets it.  Gap runs
keep their identity -- each casts one `ins` vote, also when a shift by the whole '=' run makes it abut another gap run; the junction
`len` still has no counters; everything is still an integer sum.  Only the votes change: the runs handed out stay as traced.

Properties (tests/test_normalize_cpu.py):
  (a) canonical position: two alignments that differ only in where a gap sits inside its neighbouring '=' runs vote identically;
  (b) presentation independence: the votes on a read do not depend on whether the pair presents it as V, as H on strand 0 or as H on
      strand 1 (for the last: runs reversed, I and D swapped, sequences reverse-complemented);
  (c) idempotence: the normalised alignment has all shifts 0;
  (d) conservation: the number of base + del votes is unchanged; `ins` votes differ only by the junction-`len` drops."""
from __future__ import annotations

import numpy as np

from . import pileup_mirror as P
from .trace_mirror import oriented

EQ, X, INS, DEL = 0, 1, 2, 3


def shifts(words, tbegV: int, tbegH: int, seqV: bytes, seqHp: bytes):
    """(sL, sR): int64 arrays, one entry per run of `words` (0 for runs that are no gap).  seqHp is H' (already oriented).
    All gap runs advance together, one compared base pair per step, until the last one has met a mismatch or the end of its '=' run."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    ln, op = w >> 4, w & 15
    n = len(w)
    dv, dh = np.where(op != DEL, ln, 0), np.where(op != INS, ln, 0)
    vs, hs = int(tbegV) + np.cumsum(dv) - dv, int(tbegH) + np.cumsum(dh) - dh
    SS = np.concatenate([P.codes(seqV), P.codes(seqHp)]).astype(np.int64)      # S = V or H': one array, two bases
    sL, sR = np.zeros(n, np.int64), np.zeros(n, np.int64)
    g = np.flatnonzero((op >= INS) & (ln > 0))
    if not len(g):
        return sL, sR
    isI = op[g] == INS
    x, L = np.where(isI, vs[g], hs[g]), ln[g]
    base, lenS = np.where(isI, 0, len(seqV)), np.where(isI, len(seqV), len(seqHp))
    prev_eq = (g >= 1) & (op[np.maximum(g - 1, 0)] == EQ)
    next_eq = (g + 1 < n) & (op[np.minimum(g + 1, n - 1)] == EQ)
    # a comparison stays inside S: S[x-1-t] needs t < x, S[x+L+t] needs t < lenS - x - L
    dl = np.where(prev_eq & (x >= 0) & (x + L <= lenS), np.minimum(ln[np.maximum(g - 1, 0)], np.maximum(x, 0)), 0)
    dr = np.where(next_eq & (x >= 0) & (x + L < lenS), np.minimum(ln[np.minimum(g + 1, n - 1)], np.maximum(lenS - x - L, 0)), 0)
    for d, out, lo, step in ((dl, sL, x - 1, -1), (dr, sR, x, 1)):
        s = np.zeros(len(g), np.int64)
        act = np.flatnonzero(d > 0)
        t = 0
        while len(act):
            at = base[act] + lo[act] + step * t
            act = act[SS[at] == SS[at + L[act]]]
            s[act] += 1
            act = act[s[act] < d[act]]
            t += 1
        out[g] = s
    return sL, sR


def normalized_words(words, sh, right: bool = False) -> np.ndarray:
    """A_L (right=False, sh = sL) or A_R (right=True, sh = sR) as run words.  Gap runs stay runs of their own; the '=' columns a gap
    jumped over become a run of their own next to it and the neighbour it took them from may be left with length 0 (the word 0), so
    adjacent runs may have equal ops here: pileup_mirror.votes treats every word as one run, which is what the definition asks."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    out = []
    n = len(w)
    for k in range(n):
        word = int(w[k])
        if (word & 15) == EQ:
            take = int(sh[k - 1]) if (right and k >= 1) else int(sh[k + 1]) if (not right and k + 1 < n) else 0
            out.append((((word >> 4) - take) << 4) | EQ)
        elif (word & 15) >= INS and sh[k]:
            moved = (int(sh[k]) << 4) | EQ
            out += [moved, word] if right else [word, moved]
        else:
            out.append(word)
    return np.asarray(out, np.uint32)


def votes(ops, trace, seqH: bytes, seqV: bytes, strand: int):
    """pileup_mirror.votes with every gap run at its canonical position: ((posV, ctrV), (posH, ctrH), dropped, stats).
    stats: dict(runs, gap_runs, shifted_runs, shifted_columns) of the pair as bella_vote_stats counts them -- per gap run sL for V and
    sL (strand 0) or sR (strand 1) for H."""
    o0, n = int(trace["op_off"]), int(trace["nops"])
    w = np.asarray(ops[o0:o0 + n], np.uint32)
    sL, sR = shifts(w, trace["tbegV"], trace["tbegH"], seqV, oriented(seqH, strand))
    tr = dict(op_off=0, tbegV=int(trace["tbegV"]), tbegH=int(trace["tbegH"]))
    wl = normalized_words(w, sL)
    (pV, cV), (pH, cH), _ = P.votes(wl, dict(tr, nops=len(wl)), seqH, seqV, strand)
    sH = sL
    if strand:
        wr = normalized_words(w, sR, right=True)
        _, (pH, cH), _ = P.votes(wr, dict(tr, nops=len(wr)), seqH, seqV, strand)
        sH = sR
    lenV, lenH = len(seqV), len(seqH)
    gaps = (w & 15) >= INS
    # dropped = the ins votes that fell on a junction `len`: one per gap run minus the ins votes cast
    dropped = int(gaps.sum()) - int((cV >= P.INS).sum()) - int((cH >= P.INS).sum())
    assert dropped >= 0 and (pV < lenV).all() and (pH < lenH).all()
    stats = dict(runs=n, gap_runs=int(gaps.sum()), shifted_runs=int((sL > 0).sum() + (sH > 0).sum()), shifted_columns=int(sL.sum() + sH.sum()))
    return (pV, cV), (pH, cH), dropped, stats


def pileup(reads, pairs, alns, traces, ops):
    """The normalised table of a read set, as pileup_mirror.pileup builds the plain one: (table uint32 (total bases, 9), stats dict with
    pairs, runs, gap_runs, shifted_runs, shifted_columns, votes summed over the records with nops > 0)."""
    lens = np.array([len(s) for s in reads], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = []
    tot = dict(pairs=0, runs=0, gap_runs=0, shifted_runs=0, shifted_columns=0, votes=0)
    for n in np.flatnonzero(traces["nops"] > 0):
        rid, cid, strand = int(pairs[n]["rid"]), int(pairs[n]["cid"]), int(alns[n]["strand"])
        (pV, cV), (pH, cH), _, st = votes(ops, traces[n], reads[rid], reads[cid], strand)
        flat.append((off[cid] + pV) * P.NCOUNTERS + cV)
        flat.append((off[rid] + pH) * P.NCOUNTERS + cH)
        tot["pairs"] += 1
        tot["votes"] += len(pV) + len(pH)
        for k, v in st.items():
            tot[k] += v
    idx = np.concatenate(flat).astype(np.int64) if flat else np.zeros(0, np.int64)
    table = np.bincount(idx, minlength=int(off[-1]) * P.NCOUNTERS).reshape(int(off[-1]), P.NCOUNTERS)
    return table.astype(np.uint32), tot


def derive_h(seqV: bytes, words, tbegV: int, tbegH: int, rng, lenH: int = None, dseq: bytes = b"") -> bytes:
    """H' for which `words` is a true alignment of V from (tbegV, tbegH): '=' columns copy V, 'X' columns take another base, 'D' bases
    and everything outside the alignment are random, the 'D' bases taken from `dseq` while it lasts (tests build their cases from V and
    the runs with this)."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    acgt = b"ACGT"
    out = [acgt[rng.integers(4)] for _ in range(tbegH)]
    i, nd = tbegV, 0
    for word in w:
        g, L = int(word & 15), int(word >> 4)
        for _ in range(L):
            if g == EQ:
                out.append(seqV[i]); i += 1
            elif g == X:
                out.append(acgt[(acgt.index(seqV[i]) + 1 + rng.integers(3)) % 4]); i += 1
            elif g == INS:
                i += 1
            elif nd < len(dseq):
                out.append(dseq[nd]); nd += 1
            else:
                out.append(acgt[rng.integers(4)])
    while lenH is not None and len(out) < lenH:
        out.append(acgt[rng.integers(4)])
    return bytes(out)
