"""Hand-made pairs for the banded traces and their expectation from the banded mirror.  Test tooling.

One deterministic read set: every case is a pair (H = read 2c, V = read 2c + 1) with an explicit seed and an explicit alignment
rectangle, built from a left part, k seed columns and a right part.  The families: gradual drift (one extra base every 6, enough to
walk the path onto an edge of 256, 512 and 1,024 diagonals), block insertions of 128 and 140 bases, tall and flat rectangles, empty
sides, homopolymers / dinucleotide / unit repeats (ties), seeds that mismatch at their first or last column (seams).  expectations()
runs trace_expect_banded over the list for every first band of BAND0S; coverage() is what the list must exercise, computed from
the mirror's bookkeeping alone."""
from __future__ import annotations

import multiprocessing as mp
import os

import numpy as np

from . import synth
from . import trace_mirror as M

K = 17
SEED = 20240927          # a seed at which every drift case walks onto its edge (with about one seed in ten a drift's best in-band cell lies short of it, and
                         # the side then stays narrow and short of the optimum, as the block insertions do: coverage() would still hold, the family's purpose not)
BAND0S = (0, 300, 1024, 2048, 1 << 18)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes()


def _other(rng, c):
    return bytes([[x for x in b"ACGT" if x != c][int(rng.integers(0, 3))]])


def _subs(rng, t, rate):
    """t with substitutions only (the diagonal stays where it is)"""
    return b"".join(_other(rng, c) if rng.random() < rate else bytes([c]) for c in t)


def _noisy(rng, t, rate):
    """t with substitutions, insertions and deletions, a third of the rate each"""
    out = []
    for c in t:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(_other(rng, c) if u < 2 * rate / 3 else bytes([c]))
        if u > 1 - rate / 3:
            out.append(_rand(rng, 1))
    return b"".join(out)


def _drift(rng, total, tail):
    """(plain, drifted), read away from the seed: `total` single extra bases, one after every 6 bases, then `tail` bases alike"""
    t = _rand(rng, 6 * total + tail)
    d = b"".join(t[6 * q:6 * q + 6] + _rand(rng, 1) for q in range(total)) + _subs(rng, t[6 * total:], 0.03)
    return t, d


def _block(rng, size, length=1200):
    """(plain, with one insertion of `size` bases in the middle)"""
    t = _rand(rng, length)
    return t, t[:length // 2] + _rand(rng, size) + t[length // 2:]


class Case:
    def __init__(self, name, H, V, seedH, seedV, strand, aln):
        self.name, self.H, self.V, self.seedH, self.seedV, self.strand, self.aln = name, H, V, seedH, seedV, strand, aln


def _case(rng, name, strand, left, seed, right, open_left=True, open_right=True):
    """left / right: (h, v) read away from the seed; seed: (h, v) of K columns.  The rectangle is exactly the two parts; a read whose
    length would be a multiple of 16 gets one more base outside the rectangle (at the right end if open_right, else at the left)."""
    (lh, lv), (sh, sv), (rh, rv) = left, seed, right
    assert len(sh) == len(sv) == K
    parts = []
    for l, s, r in ((lh, sh, rh), (lv, sv, rv)):
        body, pre = l[::-1] + s + r, 0
        if len(body) % 16 == 0:
            if open_right:
                body += _rand(rng, 1)
            else:
                assert open_left
                body, pre = _rand(rng, 1) + body, 1
        parts.append((body, pre, pre + len(l)))
    (Hp, preH, sH), (V, preV, sV) = parts
    aln = dict(begH=preH, endH=sH + K + len(rh), begV=preV, endV=sV + K + len(rv), strand=strand)
    H = M.revcomp(Hp) if strand else Hp
    return Case(name, H, V, len(H) - sH - K if strand else sH, sV, strand, aln)


def build_cases():
    rng = np.random.default_rng(SEED)
    cases = []

    def same_seed():
        s = _rand(rng, K)
        return s, s

    def small():                                        # an ordinary short side: related sequences, all three kinds of error
        t = _rand(rng, int(rng.integers(90, 200)))
        return _noisy(rng, t, 0.12), _noisy(rng, t, 0.06)

    def put(name, side, strand, where, other=None, **kw):
        other = small() if other is None else other
        cases.append(_case(rng, name, strand, side if where == "left" else other, same_seed(), other if where == "left" else side, **kw))

    # gradual drift: V drifts towards p = 0, H towards p = B - 1
    for total in (130, 260, 520):
        for on in "VH":
            for strand, where in ((0, "right"), (1, "left")):
                t, d = _drift(rng, total, 420)
                put("drift%d%s_%s%d" % (total, on, where, strand), (t, d) if on == "V" else (d, t), strand, where)
    # both sides drift: two doublings in one repeat of the pair; then sides that stop widening in different rounds (the left side runs
    # a third time with its band unchanged)
    (t1, d1), (t2, d2) = _drift(rng, 130, 300), _drift(rng, 130, 300)
    cases.append(_case(rng, "drift_both130_0", 0, (t1, d1), same_seed(), (d2, t2)))
    (t1, d1), (t2, d2) = _drift(rng, 130, 300), _drift(rng, 260, 300)
    cases.append(_case(rng, "drift_130H_260V_1", 1, (d1, t1), same_seed(), (t2, d2)))
    # one block insertion: 128 reaches the first diagonal of 256, 140 does not
    for size in (128, 140):
        for on in "VH":
            for strand, where in (((0, "right"), (1, "left")) if (size == 128) == (on == "V") else ((1, "right"), (0, "left"))):
                t, d = _block(rng, size)
                put("block%d%s_%s%d" % (size, on, where, strand), (t, d) if on == "V" else (d, t), strand, where)
    # tall and flat rectangles: the rows stop at m + B/2; the other side empty (the seed at position 0 or at len - k)
    q = 0
    for short in (0, 1, 10):
        for tall in (True, False):
            t = _rand(rng, 1003 + 7 * q)
            long_, short_ = _subs(rng, t, 0.05), t[:short]
            side = (short_, long_) if tall else (long_, short_)
            strand, where = q & 1, ("right", "left")[(q >> 1) & 1]
            put("%s%d_%s%d" % ("tall" if tall else "flat", short, where, strand), side, strand, where, other=(b"", b""),
                open_left=where == "left", open_right=where == "right")
            q += 1
    s = _rand(rng, K)
    cases.append(Case("seed_only_reads", s, s, 0, 0, 0, dict(begH=0, endH=K, begV=0, endV=K, strand=0)))
    s = _rand(rng, K)
    a, b, c, d = (_rand(rng, x) for x in (37, 52, 41, 29))
    cases.append(Case("seed_only_rectangles", M.revcomp(a + s + b), c + s + d, len(b), len(c), 1,
                      dict(begH=len(a), endH=len(a) + K, begV=len(c), endV=len(c) + K, strand=1)))
    # ties: homopolymers, dinucleotide repeats, a repeated unit, unequal lengths; two co-optimal end cells on one anti-diagonal
    u, w = _rand(rng, 23), _rand(rng, 7)
    tie = [((b"A" * 230, b"A" * 300), (b"AC" * 155, b"AC" * 120)),
           ((b"A" * 80 + b"C" + b"A" * 150, b"A" * 100 + b"C" + b"A" * 200), (b"AC" * 60 + b"G" + b"AC" * 95, b"AC" * 50 + b"G" + b"AC" * 70)),   # gaps inside a repeat: where they go is the tie rule
           ((b"T" * 320 + _rand(rng, 30), b"T" * 210 + _rand(rng, 45)), (b"GT" * 110 + b"G", b"GT" * 150)),
           ((b"T" * 130 + b"G" + b"T" * 90, b"T" * 95 + b"G" + b"T" * 140), (b"GT" * 40 + b"A" + b"GT" * 100, b"GT" * 66 + b"A" + b"GT" * 60)),
           ((u * 8 + _rand(rng, 40), u * 12 + _rand(rng, 40)), (w * 31, w * 20 + w[:3])),
           ((_rand(rng, 3) + b"CG" * 140, b"GC" * 140), (u * 9, u * 6 + u[:11]))]
    for q, (x, y) in enumerate(tie):
        for strand in (0, 1):
            left, right = (x, y) if strand == 0 else (y, x)
            cases.append(_case(rng, "tie%d_%d" % (q, strand), strand, left, same_seed(), right))
    t = _rand(rng, 60)
    shift = (t + b"CG" * 20, t + b"GC" * 20)             # H one base ahead or V one base ahead: the same score on the same anti-diagonal
    cases.append(_case(rng, "tie_shift_right0", 0, small(), same_seed(), shift))
    cases.append(_case(rng, "tie_shift_left1", 1, shift, same_seed(), small()))
    # seams: X at the seed's first / last column next to an X of the side; '=' through both seams; a seed that is mostly X
    for strand in (0, 1):
        lt, rt, sv = _rand(rng, 180), _rand(rng, 210), _rand(rng, K)
        first = _other(rng, sv[0]) + sv[1:]
        last = sv[:-1] + _other(rng, sv[-1])
        both = _other(rng, sv[0]) + sv[1:8] + _other(rng, sv[8]) + sv[9:-1] + _other(rng, sv[-1])
        xl = (_other(rng, lt[0]) + lt[1:], lt)            # the base next to the seed mismatches as well
        xr = (_other(rng, rt[0]) + rt[1:], rt)
        cases.append(_case(rng, "seam_first_%d" % strand, strand, xl, (first, sv), (_noisy(rng, rt, 0.08), rt)))
        cases.append(_case(rng, "seam_last_%d" % strand, strand, (_noisy(rng, lt, 0.08), lt), (last, sv), xr))
        cases.append(_case(rng, "seam_equal_%d" % strand, strand, (lt, lt), (sv, sv), (rt, rt)))
        cases.append(_case(rng, "seam_xx_both_%d" % strand, strand, xl, (both, sv), xr))
        cases.append(_case(rng, "seam_all_x_%d" % strand, strand, (lt, lt), (bytes(_other(rng, c)[0] for c in sv), sv), (rt, rt)))
    return cases


def read_set(cases):
    """the reads of the cases: H of case c is read 2c, V read 2c + 1"""
    return synth.ReadSet.from_strings([s for c in cases for s in (c.H, c.V)])


class _Memo:
    """banded_extension with the results of one case kept: its sides meet the same band under several first bands"""
    def __init__(self):
        self.d = {}

    def __call__(self, h, v, B):
        key = (h, v, B)
        if key not in self.d:
            self.d[key] = M.banded_extension(h, v, B)
        return self.d[key]


def _expect_case(c):
    memo = _Memo()
    return [M.trace_expect_banded(c.H, c.V, c.seedH, c.seedV, K, c.aln, b0, ext=memo) for b0 in BAND0S]


_EXPECT = {}


def expectations(cases):
    """{band0: [(record, ops, steps) per case]}; computed once per process and list, on up to 12 forked workers"""
    key = tuple((c.name, c.H, c.V, c.seedH, c.seedV, c.strand, tuple(sorted(c.aln.items()))) for c in cases)
    if key not in _EXPECT:
        with mp.get_context("fork").Pool(min(12, os.cpu_count() or 1)) as pool:
            per_case = pool.map(_expect_case, cases, chunksize=1)
        _EXPECT[key] = {b0: [r[q] for r in per_case] for q, b0 in enumerate(BAND0S)}
    return _EXPECT[key]


def bookkeeping(exp):
    """what bella_trace_stats must report after one call on the list: dict(widened_extensions, repeated_pairs, extensions)"""
    runs = sum(len(steps[0]) for _, _, steps in exp)
    return dict(widened_extensions=sum(r["widened"] for r, _, _ in exp), repeated_pairs=runs - len(exp), extensions=2 * runs)


def coverage(cases, expect):
    """Counts over every first band, from the mirror's steps: per DP the DEVICE runs, not per distinct DP -- a side that meets the same
    band under several first bands, or runs again unchanged because the other side touched, counts every time.  dict(tall[cls]: side DPs with more rows than B, touches[band]: (low
    edge, high edge), short: cases that end below their covering optimum with no widening); cls 0..3 = 256, 512, 1,024, wider."""
    tall = [0, 0, 0, 0]
    touches = {256: [0, 0], 512: [0, 0], 1024: [0, 0]}
    for b0 in BAND0S:
        for c, (_, _, steps) in zip(cases, expect[b0]):
            _, (ml, nl), (mr, nr) = M.rectangles(len(c.H), len(c.V), c.seedH, c.seedV, K, c.aln)
            for (m, n), st in zip(((ml, nl), (mr, nr)), steps):
                for band, touch in st:
                    if min(n, m + band // 2) > band:
                        tall[{256: 0, 512: 1, 1024: 2}.get(band, 3)] += 1
                    if touch and band in touches and band < M.trace_cover_band(n, m):
                        touches[band][0] += bool(touch & M.TOUCH_LOW)
                        touches[band][1] += bool(touch & M.TOUCH_HIGH)
    short = sum(1 for b0 in BAND0S[:-1] for (r, _, _), (rc, _, _) in zip(expect[b0], expect[BAND0S[-1]]) if r["widened"] == 0 and r["score"] < rc["score"])
    return dict(tall=tall, touches=touches, short=short)


def check_coverage(cov):
    """the conditions the list is built for; AssertionError names the one that fails"""
    assert all(x >= 8 for x in cov["tall"]), "every kernel class needs 8 side DPs with more rows than diagonals: %s" % cov["tall"]
    for band, (low, high) in cov["touches"].items():
        assert low + high >= 2 and low >= 1 and high >= 1, "touches below the cover at %d diagonals (low, high): %s" % (band, (low, high))
    assert cov["short"] >= 1, "no case ends short of its covering optimum without widening"
