"""TEST TOOLING: inputs that put k-mer counting (bella_amd/csrc/kcount.hpp) on its edges ON PURPOSE -- tile, group, 16-bit counter,
fast-path limit, look-up table, minimizer ring, small k, emission rounds, several passes.

A read of exactly k bases holds one canonical word, so a list of (word, multiplicity) fixes the array a pass sorts word for word.
Every builder lays its words out as SLOTS -- a slot is one group of the run kernels (the 2^gb neighbouring words that share
word >> gb), given as its multiplicity per low-bit value -- in ascending order, draws ascending groups whose words are their own
canonical form, writes each word in its forward or reverse-complement form at random and shuffles the reads.  What the input then
IS comes from bella_testkit/kcount_mirror.py alone: tags(case) derives the geometry from the mirror's description, the builder
names the tags it was built for (case.want) and make() raises when one is missing.  A case can therefore not miss its edge
unnoticed.  Filler words are singletons whose group neighbours are all canonical (k = 5 has too few such groups: its fillers are
groups of counts 1 and upper + 1, unreliable all the same)."""
from __future__ import annotations

import dataclasses
import itertools

import numpy as np

from . import kcount_mirror as M
from .synth import ReadSet

U64 = np.uint64
TILE, HALO = M.RUN_TILE, M.RUN_HALO


@dataclasses.dataclass
class Case:
    family: str
    name: str
    rs: ReadSet
    k: int
    lower: int = 2
    upper: int = 8
    mode: int = 0
    window: int = 0
    debug: int = 0
    budget: int = 0
    want: tuple = ()
    _desc: object = None

    def describe(self):
        if self._desc is None:
            self._desc = M.describe(self.rs, self.k, self.lower, self.upper, self.mode, self.window, self.debug, self.budget)
        return self._desc

    @property
    def syncmer(self):
        return self.mode == 1


def make(family, name, rs, k, want, **kw):
    c = Case(family, name, rs, k, want=tuple(want), **kw)
    have = tags(c)
    missing = [w for w in c.want if w not in have]
    if missing:
        raise AssertionError("%s/%s does not have the geometry it was built for: %r (has %r)" % (family, name, missing, sorted(have)[:40]))
    return c


# ---- words, groups, reads ---------------------------------------------------------------------------------------------------------

def rc_words(w, k):
    w = np.asarray(w, U64)
    r = np.zeros(w.shape, U64)
    for _ in range(k):
        r = (r << U64(2)) | (U64(3) - (w & U64(3)))
        w = w >> U64(2)
    return r


def is_canonical(w, k):
    w = np.asarray(w, U64)
    return w <= rc_words(w, k)


def pick_groups(k, gb, n, rng, b0=0, b1=M.BINS, vs=None):
    """n ascending groups (word >> gb) of the bins [b0, b1) whose words with low bits in `vs` (default: all) are canonical"""
    if n == 0:
        return np.zeros(0, U64)
    vs = tuple(range(1 << gb)) if vs is None else vs
    sh = max(2 * k - 8, 0)
    lo, hi = (b0 << sh) >> gb, ((b1 << sh) >> gb if k >= 4 else 1 << max(2 * k - gb, 0))
    if hi - lo <= 1 << 20:
        cand = np.arange(lo, hi, dtype=U64)
    else:
        cand = np.unique(U64(lo) + (rng.random(8 * n + 200000) * float(hi - lo - 4096)).astype(U64))
    ok = np.ones(len(cand), bool)
    for v in vs:
        ok &= is_canonical((cand << U64(gb)) | U64(v), k)
    cand = cand[ok]
    if len(cand) < n:
        raise AssertionError("k = %d, bins [%d, %d): %d groups with canonical words, %d needed" % (k, b0, b1, len(cand), n))
    return np.sort(rng.choice(cand, n, replace=False))


def realise(k, gb, segments, rng):
    """segments: [(first bin, end bin, allowed low bits or None, slots)] in ascending bin order -> (words, multiplicities)"""
    words, mults = [], []
    for b0, b1, vs, slots in segments:
        for g, slot in zip(pick_groups(k, gb, len(slots), rng, b0, b1, vs), slots):
            assert len(slot) == 1 << gb and (vs is None or all(v in vs for v, c in enumerate(slot) if c))
            for v, c in enumerate(slot):
                if c:
                    words.append((int(g) << gb) | v)
                    mults.append(int(c))
    return np.asarray(words, U64), np.asarray(mults, np.int64)


def reads_of(k, words, mults, rng, strands=True, prefix=0, last_word=None):
    """one read of k (+ prefix) bases per copy of a word, either strand at random, shuffled (last_word: its first copy goes last)"""
    w = np.repeat(np.asarray(words, U64), mults)
    n = len(w)
    x = np.where(rng.random(n) < 0.5, rc_words(w, k), w) if strands else w
    sh = (2 * (k - 1 - np.arange(k))).astype(U64)
    codes = ((x[:, None] >> sh[None, :]) & U64(3)).astype(np.uint8)
    if prefix:
        codes = np.concatenate([rng.integers(0, 4, (n, prefix), dtype=np.uint8), codes], 1)
    perm = rng.permutation(n)
    if last_word is not None:
        at = int(np.flatnonzero(w[perm] == U64(last_word))[0])
        perm[[at, n - 1]] = perm[[n - 1, at]]
    codes = codes[perm]
    L = k + prefix
    return ReadSet(codes.reshape(-1), np.arange(n + 1, dtype=np.int64) * L, ["r%d" % i for i in range(n)])


def run(gb, n, v=0):
    """a slot with n words of low bits v"""
    s = [0] * (1 << gb)
    s[v % (1 << gb)] = n
    return tuple(s)


def fillers(gb, n, rng, fat=0):
    """slots of n unreliable words: singletons, or (fat = upper + 1) few groups of counts 1 and fat"""
    if not fat or gb == 0:
        return [run(gb, 1, int(rng.integers(0, 4))) for _ in range(n)]
    out = []
    while n > 0:
        big = min(n // fat, 4)
        one = min(n - big * fat, 4 - big)
        out.append(tuple([fat] * big + [1] * one + [0] * (4 - big - one)))
        n -= big * fat + one
    return out


def place(gb, total, placed, rng, fat=0):
    """slots of `total` words with the given slots at the given places of the sorted array and fillers in between"""
    out, at = [], 0
    for x, slot in sorted(placed, key=lambda p: p[0]):
        if x < at:
            raise AssertionError("slots overlap at %d" % x)
        out += fillers(gb, x - at, rng, fat) + [slot]
        at = x + sum(slot)
    if at > total:
        raise AssertionError("%d words placed, %d allowed" % (at, total))
    return out + fillers(gb, total - at, rng, fat)


def one_pass(k, slots, rng, **kw):
    fast, pb, gb = M.plan(sum(sum(s) for s in slots), k, 0)
    w, m = realise(k, gb, [(0, M.BINS, None, slots)], rng)
    return reads_of(k, w, m, rng, **kw)


def gb_of(k):
    return M.plan(1000, k, 0)[2]


# ---- what an input is, read from the mirror ---------------------------------------------------------------------------------------

EDGE_E = (0, 1, 2015, 2016, 2046, 2047)
TOTALS = (1, 2, 2047, 2048, 2049, 2080, 2081, 4096, 4097)


def tags(c: Case):
    """the geometry of a case as a set of strings, from the mirror's description alone"""
    d = c.describe()
    cd = d["counted"]
    k, t = c.k, set()
    t.add("path:%s" % ("fast" if d["fast"] else "lookup"))
    t.add("plan:k%d:n%d:%s" % (k, cd.npositions, "fast" if d["fast"] else "lookup"))
    ps = d["passes"]
    budget = c.budget or 1 << 30
    if len(ps) >= 3:
        t.add("passes>=3")
    for i, (b0, b1, n) in enumerate(ps):
        if n > budget and b1 == b0 + 1:
            t.add("pass:over-budget")
        if n == 0 and any(p[2] for p in ps[:i]) and any(p[2] for p in ps[i + 1:]):
            t.add("pass:zero-between")
    bins = np.unique(M.code_bin(cd.counted_words, k)) if len(cd.counted_words) else np.zeros(0, np.int64)
    if len(ps) >= 3 and bins.tolist() == [0, 255]:
        t.add("pass:bins-0-255")
    if 2 * k + d["pb"] == 64 and len(cd.codes) and int(cd.codes[-1]) >> (2 * k - 2) == 3:
        t.add("key:bit63")
    if len(cd.t_kmer) and int(cd.t_read[-1]) == c.rs.nreads - 1 and int(cd.t_pos[-1]) == int(c.rs.lengths[-1]) - k:
        t.add("tuple:last-position")
    if d["pb"] and cd.npositions == 1 << d["pb"]:
        t.add("positions:field-full")
    for (b0, b1, n), L in zip(ps, d["layouts"]):
        if L is None:
            continue
        if n in TOTALS:
            t.add("total:%d" % n)
        last_tile = np.arange(L.ntiles) * TILE + L.have == n
        if L.ntiles and L.have[-1] < TILE:
            t.add("tile:last-partial")
        rel = L.mask != 0
        for e in EDGE_E:
            if np.any(rel & (L.e == e)):
                t.add("head:e%d" % e)
            if np.any(rel & (L.e == e) & (L.tile > 0)):
                t.add("head:e%d:inner-tile" % e)
        for off in (-1, 0, 1):
            for where, sel in (("last", last_tile[L.tile]), ("inner", ~last_tile[L.tile])):
                if np.any(rel & (L.end == off) & sel & (L.length > 2)):
                    t.add("end:%s:%+d" % (where, off))
        if np.any(L.bisects & (L.end == 0)):
            t.add("bisect:zero-extra")
        head_at = set(L.start.tolist())
        for tl in range(1, L.ntiles):
            if tl * TILE in head_at:
                t.add("tile-start:fresh")
            else:
                owner = int(np.searchsorted(L.start, tl * TILE, side="right") - 1)
                if L.mask[owner]:
                    t.add("tile-start:continued")
        # a group that fills whole tiles: the tiles in between have no head at all
        nohead = np.flatnonzero(np.bincount(L.tile, minlength=L.ntiles) == 0)
        if len(nohead) >= 2:
            t.add("tiles:headless>=2")
        for r in np.unique(L.tile_rec):
            t.add("rec:%d" % r)
        if np.any((L.tile_rec[:-1] == TILE // 2) & (L.tile_rec[1:] == TILE // 2)):
            t.add("rec:1024:twice-in-a-row")
        if d["gb"] == 2:
            nr = (L.mask[:, None] >> np.arange(4) & 1).sum(1)
            for i in np.flatnonzero(rel):
                m, cn = int(L.mask[i]), L.cnt[i]
                oth = [int(cn[v]) for v in range(4) if not (m >> v) & 1]
                kinds = [kd for kd, okk in (("absent", all(x == 0 for x in oth)), ("low", all(x == 1 for x in oth)),
                                            ("high", all(x == c.upper + 1 for x in oth))) if okk]
                blk = (L.tile == L.tile[i]) & (L.e // 64 == L.e[i] // 64) & (L.e < L.e[i])
                planes = int(np.bitwise_or.reduce(nr[blk])) if blk.any() else 0
                for kd in kinds:
                    t.add("mask:k%d:%d:%s" % (k, m, kd))
                if bin(planes).count("1") >= 2:
                    t.add("mask:k%d:%d:planes>=2" % (k, m))
                if planes == 7:
                    t.add("mask:k%d:%d:planes=7" % (k, m))
                if L.e[i] & 63 in (0, 63):
                    t.add("mask:k%d:%d:a%d" % (k, m, L.e[i] & 63))
        big = np.argwhere(L.cnt >= 65535)
        for i, v in big:
            n16 = int(L.cnt[i, v])
            t.add("big:v%d:%d:u%d" % (v, n16, c.upper))
            if bin(int(L.mask[i]) & ~(1 << v)).count("1"):
                t.add("big:%d:reliable-neighbour" % n16)
            if i + 1 < len(L.start):
                t.add("big:next-head:e%d" % int(L.e[i + 1]))
            if (int(L.start[i]) + int(L.length[i])) // TILE - int(L.tile[i]) >= 3:
                t.add("big:whole-tiles-inside>=2")
            if int(L.start[i]) + int(L.length[i]) == n and len(ps) > 1:
                t.add("pass:ends-after-big-bin")
    if c.mode and len(cd.counted_words):
        u, r = np.unique(cd.counted_words, return_counts=True)
        for w, n in zip(u[r >= 65535], r[r >= 65535]):
            nb = [x for x in cd.codes.tolist() if x >> 2 == int(w) >> 2 and x != int(w)]
            t.add("sat:m%d:%d:u%d:%s" % (c.mode, n, c.upper, "with-neighbour" if nb else "alone"))
            t.add("sat:m%d:%d:u%d:%s" % (c.mode, n, c.upper, "reliable" if int(w) in set(cd.codes.tolist()) else "not-reliable"))
    if not d["fast"]:
        nk, slots = len(cd.codes), d["slots"]
        t.add("dict:%d" % nk)
        if 2 * nk == slots:
            t.add("table:load-half")
        keys = cd.codes[cd.codes != U64(M.HASH_EMPTY)]
        hm = M.home(keys, slots) if len(keys) else np.zeros(0, np.int64)
        if (hm == slots - 1).sum() >= 4:
            t.add("table:last-slot>=4")                 # four keys homed at the last slot: the chain holds slots-1, 0, 1, 2
            allw = np.unique(M.position_words(c.rs, k)[1])
            miss = allw[~np.isin(allw, keys)]
            if (M.home(miss, slots) == slots - 1).sum() >= 4:
                t.add("table:last-slot-misses>=4")
        if len(cd.codes) != len(keys):
            t.add("table:all-T-left-out")
    if cd.longest_deque is not None and len(cd.longest_deque):
        t.add("ring:k%d:w%d:r%d" % (k, c.window, c.rs.nreads))
        if int(cd.longest_deque.max()) == c.window + 1:
            t.add("ring:full")
        if int(cd.longest_deque.max()) == c.window + 1 and 2 * int(cd.longest_deque.min()) <= c.window + 2:   # a lane at half the ring or less
            t.add("ring:full-beside-short")
        nks = np.maximum(c.rs.lengths.astype(np.int64) - k + 1, 0)
        if np.all(nks == nks[0]):
            t.add("ring:w-nk:%+d" % (c.window - int(nks[0])) if abs(c.window - int(nks[0])) <= 1 else "ring:w-small")
        t.add("ring:sampled" if len(cd.counted_words) else "ring:nothing-sampled")
    cursor = c.mode != 0 or len(ps) > 1
    for nkm in np.unique(np.maximum(c.rs.lengths.astype(np.int64) - k + 1, 0)):
        if nkm in (1023, 1024, 1025, 2048, 2049) and cursor:
            t.add("emit:%d:m%d:%s" % (nkm, c.mode, "passes" if len(ps) > 1 else "one-pass"))
    return t


# ---- the families -----------------------------------------------------------------------------------------------------------------

def tile_edges(ks=(17, 16, 13)):
    out = []
    for k in ks:
        gb = gb_of(k)
        rng = np.random.default_rng(1000 + k)
        pair = lambda: run(gb, 2, int(rng.integers(0, 4)))
        for n in TOTALS:
            placed = [(0, pair())] if n >= 2 else []
            if n >= 4:
                placed.append((n - 2, pair()))
            want = ["total:%d" % n, "path:fast"] + (["tile:last-partial"] if n % TILE else [])
            out.append(make("tile_edges", "k%d-total-%d" % (k, n), one_pass(k, place(gb, n, placed, rng), rng), k, want))
        for e in EDGE_E:
            placed = [(e, pair()), (TILE + e, pair())]
            out.append(make("tile_edges", "k%d-head-e%d" % (k, e), one_pass(k, place(gb, 2 * TILE + 100, placed, rng), rng), k,
                            ["head:e%d" % e, "head:e%d:inner-tile" % e] + (["tile-start:fresh"] if e == 0 else [])))
        for off in (-1, 0, 1):
            # inner tile: have = 2,080; the group starts at e = 2,000 of tile 0 and the pass goes on behind the look-ahead
            ln = TILE + HALO - 2000 + off
            out.append(make("tile_edges", "k%d-end-inner%+d" % (k, off), one_pass(k, place(gb, 2 * TILE + 50, [(2000, run(gb, ln, 1))], rng), rng), k,
                            ["end:inner:%+d" % off] + (["bisect:zero-extra"] if off == 0 else []), upper=200))
        for off in (-1, 0):
            # last tile (have = the words that are left): a group cannot end past it
            n = TILE + 300
            ln = 60
            out.append(make("tile_edges", "k%d-end-last%+d" % (k, off), one_pass(k, place(gb, n, [(n - ln + off, run(gb, ln, 2))], rng), rng), k,
                            ["end:last:%+d" % off, "tile:last-partial"], upper=200))
        out.append(make("tile_edges", "k%d-tile1-continued" % k, one_pass(k, place(gb, 2 * TILE + 7, [(TILE - 3, run(gb, 7, 3))], rng), rng), k,
                        ["tile-start:continued"]))
    return out


PRE = {0: [], 3: [(2, 0, 0, 0), (0, 2, 2, 0)], 7: [(0, 0, 2, 0), (2, 0, 0, 2), (2, 2, 2, 2)]}


def _mask_slot(m, kind, upper):
    other = {"absent": 0, "low": 1, "high": upper + 1}[kind]
    return tuple((2 + (v + m) % 3) if (m >> v) & 1 else other for v in range(4))


def masks(ks=(17, 13, 5)):
    out = []
    for k in ks:
        gb = gb_of(k)
        assert gb == 2
        rng = np.random.default_rng(2000 + k)
        per_set = 15 if k > 5 else 3
        for kind, pre, a in itertools.product(("absent", "low", "high"), (0, 3, 7), (20, 0, 63)):
            for m0 in range(1, 16, per_set):
                placed, want = [], []
                for j, m in enumerate(range(m0, m0 + per_set)):
                    x = 64 * (j + 1) + a
                    back = x
                    for s in reversed(PRE[pre]):
                        back -= sum(s)
                        placed.append((back, s))
                    placed.append((x, _mask_slot(m, kind, 8)))
                    want.append("mask:k%d:%d:%s" % (k, m, kind))
                    if pre == 7 and a:
                        want.append("mask:k%d:%d:planes=7" % (k, m))
                    if pre and a:
                        want.append("mask:k%d:%d:planes>=2" % (k, m))
                    if a != 20:
                        want.append("mask:k%d:%d:a%d" % (k, m, a))
                slots = place(gb, 64 * (per_set + 2), placed, rng, fat=9 if k == 5 else 0)
                out.append(make("masks", "k%d-%s-pre%d-a%d-m%d" % (k, kind, pre, a, m0), one_pass(k, slots, rng), k, want))
    return out


def dense(k=17):
    gb, rng = gb_of(k), np.random.default_rng(3000)
    pairs = lambda n: [run(gb, 2, int(rng.integers(0, 4))) for _ in range(n)]
    return [make("dense", "1024-pairs", one_pass(k, pairs(1024), rng), k, ["rec:1024", "total:2048"]),
            make("dense", "1023-pairs-2-singles", one_pass(k, pairs(500) + fillers(gb, 1, rng) + pairs(523) + fillers(gb, 1, rng), rng), k,
                 ["rec:1023", "total:2048"]),
            make("dense", "2048-pairs", one_pass(k, pairs(2048), rng), k, ["rec:1024:twice-in-a-row", "total:4096"])]


def _long_slots(gb, rng, before=2047, big=65538, v=2, after=552):
    g = [2, 3, 2]
    g.insert(v, big)
    return fillers(gb, before, rng) + [tuple(g)] + [run(gb, 2, int(rng.integers(0, 4))) for _ in range(after)]


def long_runs(k=17):
    gb, out = gb_of(k), []
    rng = np.random.default_rng(4000)
    for v in (2, 0, 3):
        out.append(make("long_runs", "base-v%d" % v, one_pass(k, _long_slots(gb, rng, v=v), rng), k,
                        ["big:v%d:65538:u8" % v, "big:65538:reliable-neighbour", "big:whole-tiles-inside>=2", "tiles:headless>=2"]))
    for e, before in ((0, 2039), (1, 2040)):                              # 2,039 + 65,545 = 33 tiles exactly
        out.append(make("long_runs", "next-head-e%d" % e, one_pass(k, _long_slots(gb, rng, before=before, after=40), rng), k,
                        ["big:next-head:e%d" % e, "big:whole-tiles-inside>=2", "tiles:headless>=2"]))
    for big in (65535, 65536, 65537, 65538):
        out.append(make("long_runs", "count-%d-u65535" % big, one_pass(k, _long_slots(gb, rng, before=100, big=big, after=40), rng), k,
                        ["big:v2:%d:u65535" % big, "big:%d:reliable-neighbour" % big], upper=65535))
    return out


def _a_syncmer_pair(k, rng):
    """two canonical neighbouring words (low bits 0 and 1 of one group) that are both syncmers"""
    g = pick_groups(k, 2, 4000, rng)
    ok = M.is_syncmer(g << U64(2), k) & M.is_syncmer((g << U64(2)) | U64(1), k)
    return int(g[ok][0]) << 2


def saturation(k=17):
    out = []
    rng = np.random.default_rng(5000)
    for mode in (2, 1):
        w0 = _a_syncmer_pair(k, rng) if mode == 1 else int(pick_groups(k, 2, 1, rng)[0]) << 2
        for big in (65535, 65536, 65537, 65538):
            fill, fm = realise(k, 2, [(0, M.BINS, None, fillers(2, 30, rng))], rng)
            words = np.concatenate([fill, np.asarray([w0, w0 + 1], U64)])
            mults = np.concatenate([fm, [big, 3]])
            rs = reads_of(k, words, mults, rng, strands=mode == 2, prefix=1 if mode == 2 else 0)
            for upper in (65535, 65534):
                out.append(make("saturation", "m%d-%d-u%d" % (mode, big, upper), rs, k,
                                ["sat:m%d:%d:u%d:with-neighbour" % (mode, big, upper),
                                 "sat:m%d:%d:u%d:%s" % (mode, big, upper, "reliable" if upper == 65535 else "not-reliable")],
                                upper=upper, mode=mode, window=1 if mode == 2 else 0))
    return out


def fast_limit():
    out = []
    rng = np.random.default_rng(6000)
    for k, limit in ((25, 16384), (24, 65536), (31, 4), (29, 64)):
        gb = M.plan(limit, k, 0)[2]
        for n in (limit, limit + 1):
            npair = min(n // 2, 40)
            top = max(1, npair // 4)                                  # reliable pairs whose top base is T
            segs = [(0, 192, None, [run(gb, 2, 0) for _ in range(npair - top)] + fillers(gb, n - 2 * npair, rng)),
                    (192, 256, (0,), [run(gb, 2, 0) for _ in range(top)])]
            w, m = realise(k, gb, segs, rng)
            rs = reads_of(k, w, m, rng, last_word=int(w[-1]))
            fast = n == limit
            out.append(make("fast_limit", "k%d-%d" % (k, n), rs, k, ["plan:k%d:n%d:%s" % (k, n, "fast" if fast else "lookup"), "tuple:last-position"] +
                            (["key:bit63", "positions:field-full"] if fast else [])))
    return out


def _homed(k, slots, n, rng, syncmer=False, taken=()):
    """n canonical words whose home slot is the table's last"""
    got = []
    while len(got) < n:
        g = pick_groups(k, 0, 40000, rng)
        g = g[M.home(g, slots) == slots - 1]
        if syncmer:
            g = g[M.is_syncmer(g, k)]
        got += [int(x) for x in g if int(x) not in taken and int(x) not in got]
    return got[:n]


def lookup():
    out = []
    rng = np.random.default_rng(7000)
    for name, k, mode, debug in (("debug14-k17", 17, 0, M.DEBUG_LOOKUP), ("k32", 32, 0, 0), ("syncmers-k17", 17, 1, 0)):
        for nd in (511, 512, 513, 1024, 1025):
            slots = M.table_slots(nd)
            rel = _homed(k, slots, 4, rng, mode == 1) if nd == 512 else []
            unrel = _homed(k, slots, 4, rng, mode == 1, rel) if nd == 512 else []
            cand = pick_groups(k, 0, 20 * nd + 3000, rng)
            if mode == 1:
                cand = cand[M.is_syncmer(cand, k)]
            cand = [int(x) for x in rng.permutation(cand) if int(x) not in rel and int(x) not in unrel]
            assert len(cand) >= nd + 200
            words = np.asarray(rel + cand[:nd - len(rel)] + unrel + cand[nd:nd + 200], U64)
            mults = np.asarray([2 + i % 3 for i in range(nd)] + [1] * (len(words) - nd), np.int64)
            rs = reads_of(k, words, mults, rng, strands=mode != 1)
            want = ["dict:%d" % nd, "path:lookup"] + (["table:load-half"] if nd in (512, 1024) else [])
            if nd == 512:
                want += ["table:last-slot>=4", "table:last-slot-misses>=4"]
            out.append(make("lookup", "%s-dict-%d" % (name, nd), rs, k, want, mode=mode, debug=debug, upper=8))
    for acopies in (3, 1):
        seqs = ["T" * 32] * 3 + ["A" * 32] * acopies + ["ACGT" * 8] * 2 + ["T" * 16 + "A" * 16] * 2 + ["ACGTTGCA" * 4]
        order = rng.permutation(len(seqs))
        rs = ReadSet.from_strings([seqs[i] for i in order])
        out.append(make("lookup", "syncmers-k32-allT-allA-x%d" % acopies, rs, 32, ["table:all-T-left-out", "path:lookup"], mode=1))
    return out


def _periodic_reads(k, nk, rng):
    L = k + nk - 1
    rep = lambda unit: (unit * (L // len(unit) + 1))[:L]
    rand = "".join("ACGT"[i] for i in rng.integers(0, 4, L))
    return [rep("A"), rep("AT"), rep("T"), rep("ACG"), rep("C"), rep("AACT"), rep("G"), rep("TA"), rep("CG")], rand


def minimizer_ring(ks=(17, 5), nk=40):
    out = []
    for k in ks:
        rng = np.random.default_rng(8000 + k)
        per, rand = _periodic_reads(k, nk, rng)
        for window, nreads in itertools.product((1, 2, 3, 10, nk - 1, nk, nk + 1), (1, 63, 64, 65, 129)):
            rs = ReadSet.from_strings([per[i % len(per)] for i in range(nreads)])
            want = ["ring:k%d:w%d:r%d" % (k, window, nreads)]
            want += ["ring:full", "ring:w-small"] if window <= 10 else ["ring:w-nk:%+d" % (window - nk)]
            want += ["ring:nothing-sampled"] if window >= nk else ["ring:sampled"]
            out.append(make("minimizer_ring", "k%d-w%d-r%d" % (k, window, nreads), rs, k, want, mode=2, window=window, upper=65535))
        mixed = [per[0], rand, per[1], rand, per[2], per[3], rand[::-1], per[5]] * 9
        out.append(make("minimizer_ring", "k%d-mixed" % k, ReadSet.from_strings(mixed), k, ["ring:full-beside-short"], mode=2, window=10, upper=65535))
    return out


def _all_strings(L, rng, strand_free=True):
    n = 4 ** L
    mult = rng.integers(0, 6, n)
    w = np.repeat(np.arange(n, dtype=U64), mult)
    sh = (2 * (L - 1 - np.arange(L))).astype(U64)
    codes = ((w[:, None] >> sh[None, :]) & U64(3)).astype(np.uint8)
    codes = codes[rng.permutation(len(w))]
    return ReadSet(codes.reshape(-1), np.arange(len(w) + 1, dtype=np.int64) * L, ["r%d" % i for i in range(len(w))])


def small_k():
    out = []
    rng = np.random.default_rng(9000)
    for k in range(1, 7):
        out.append(make("small_k", "all-k%d" % k, _all_strings(k, rng), k, ["path:fast"], upper=6 if k > 2 else 65535))
    for k in (6, 7):
        out.append(make("small_k", "syncmers-k%d" % k, _all_strings(k, rng), k, ["path:lookup"], mode=1, upper=4))
    for k, window, extra in itertools.product(range(1, 6), (1, 2), (1, 2)):
        out.append(make("small_k", "minimizers-k%d-w%d-len+%d" % (k, window, extra), _all_strings(k + extra, rng), k, ["path:fast"], mode=2,
                        window=window, upper=65535 if k < 4 else 40))
    return out


def emit_chunks(k=17):
    rng = np.random.default_rng(10000)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs = []
    for nk in (1023, 1024, 1025, 2048, 2049):
        s = bytes(b"ACGT"[i] for i in rng.integers(0, 4, k + nk - 1))
        seqs += [s, s[::-1].translate(comp), b"AT" * 30]
    rs = ReadSet.from_strings(seqs)
    out = []
    for name, mode, window, budget in (("minimizers", 2, 5, 0), ("minimizers-budget", 2, 5, 700), ("all-budget", 0, 0, 2000)):
        want = ["emit:%d:m%d:%s" % (nk, mode, "passes" if budget else "one-pass") for nk in (1023, 1024, 1025, 2048, 2049)]
        out.append(make("emit_chunks", name, rs, k, want + (["passes>=3"] if budget else []), mode=mode, window=window, budget=budget))
    return out


def _multi(name, k, slots_mid, rng, want, upper=8):
    """bin 0 within the budget | bin 20 over it (the slots under test) | nothing | bin 40 over it | bin 255: five passes.  (A group whose
    four words are all canonical begins with A: such groups stand in the bins below 64.)"""
    gb = gb_of(k)
    budget = 400
    assert sum(sum(s) for s in slots_mid) > budget
    first = fillers(gb, 300, rng) + [run(gb, 2, 1)] * 3
    third = fillers(gb, 450, rng) + [run(gb, 3, 2)] * 2
    segs = [(0, 1, None, first), (20, 21, None, slots_mid), (40, 41, None, third), (255, 256, (0,), [run(gb, 2, 0), run(gb, 1, 0)])]
    w, m = realise(k, gb, segs, rng)
    return make("multi_pass", name, reads_of(k, w, m, rng), k, ["passes>=3", "pass:over-budget", "pass:zero-between"] + want, upper=upper, budget=budget)


def multi_pass(k=17):
    gb, out = gb_of(k), []
    rng = np.random.default_rng(11000)
    pair = lambda: run(gb, 2, int(rng.integers(0, 4)))
    out.append(_multi("tile-edges", k, place(gb, 2 * TILE + 7, [(0, pair()), (2016, pair()), (TILE - 1, run(gb, 5, 3)), (TILE + 2046, pair())], rng), rng,
                      ["head:e0", "head:e2016", "head:e2047", "head:e2046:inner-tile", "tile:last-partial"]))
    out.append(_multi("tile-edges-end", k, place(gb, 2 * TILE + 50, [(2000, run(gb, TILE + HALO - 2000, 1))], rng), rng, ["end:inner:+0", "bisect:zero-extra"],
                      upper=200))
    placed, want = [], []
    for j, m in enumerate(range(1, 16)):
        x = 64 * (j + 1) + 20
        back = x
        for s in reversed(PRE[7]):
            back -= sum(s)
            placed.append((back, s))
        placed.append((x, _mask_slot(m, "low", 8)))
        want += ["mask:k%d:%d:low" % (k, m), "mask:k%d:%d:planes=7" % (k, m)]
    out.append(_multi("masks", k, place(gb, 64 * 17, placed, rng), rng, want))
    out.append(_multi("long-runs", k, _long_slots(gb, rng, before=2047, after=0), rng, ["big:v2:65538:u8", "pass:ends-after-big-bin", "tiles:headless>=2"]))
    # only the first and the last bin hold words; each is over the budget, the pass between them is empty
    a = fillers(gb, 500, rng) + [pair() for _ in range(30)]
    w, m = realise(k, gb, [(0, 1, None, a), (255, 256, (0,), [run(gb, 2, 0)] * 20 + [run(gb, 1, 0)] * 409)], rng)
    out.append(make("multi_pass", "bins-0-255", reads_of(k, w, m, rng), k, ["pass:bins-0-255", "passes>=3", "pass:zero-between"], budget=400))
    return out


FAMILIES = {"tile_edges": tile_edges, "masks": masks, "dense": dense, "long_runs": long_runs, "saturation": saturation, "fast_limit": fast_limit,
            "lookup": lookup, "minimizer_ring": minimizer_ring, "small_k": small_k, "emit_chunks": emit_chunks, "multi_pass": multi_pass}
_built = {}


def family(name):
    """the cases of a family, built once per process"""
    if name not in _built:
        _built[name] = FAMILIES[name]()
    return _built[name]
