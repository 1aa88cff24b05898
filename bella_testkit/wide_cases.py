"""Read sets whose pairs sit on the edges of the path above the LDS tiers (bella_amd/csrc/wide.hpp: the fold classes of
k_wide_fold_wg, the position grid, the LDS grouping of k_wide_group1 / k_wide_group2_chunks).  Test tooling: nothing here is used
by the product.  Laid out like the Q sets of tier_cases.py -- at least 1,024 reads, every hub on an id the assembly-time sample does
not see, the sampled ballast column -- so that the sample calls the input neither pair-rich nor long-list and no row lists are built
on their own (asserted in _finish).

A set is made of explicit tuples (kmer, read, pos) over REAL shared sequence:
    a HUB is a random read; a PARTNER carries a stretch of it, and a chosen subset of the stretch's k-mer offsets are the pair's m
    products -- the k-mers between them exist in both reads but are in no tuple, so tuples closer than k agree with the sequence and
    the strand test of the reference (string compare) and of the device (orientation bits) see the same thing.  The k-mer ids are a
    seeded random permutation of the hub's offsets: the product order is not the position order.  A partner planted as the reverse
    complement of its forward design has its positions mirrored (pos -> len - k - pos).
Layouts of a pair:
    dense    consecutive offsets, one diagonal: a plain chain (every product's parent is its successor);
    sparse   m offsets drawn without replacement from a span of 12 m (capped: reads stay <= 65,535 bases), one diagonal: a plain
             chain whose grid scans and walks go far -- `count` = m + the ancestors passed alive wraps mod 2^16;
    D diagonals   the dense stretch cut into D parts, 700 random bases between them in the partner (> binSize 500).  The estimate
             is min(begH, begV) + min(lenH - endH, lenV - endV) + k: a hub that lies inside its partner gets the same estimate on
             every diagonal, so the hub has a left flank longer than anything the partner has before a product and the partner a
             right flank longer than anything the hub has behind one -- the estimate is then (partner position) + (hub remainder) + k,
             716 apart from one part to the next: D final bins.

fold_route() restates which code of k_wide_fold_wg folds a list of m products (read from the code, wide.hpp)."""
from __future__ import annotations

import numpy as np

from . import synth
from .tier_cases import DIAGONAL_GAP, K, SPACER, _COMP, mults, regime_of, sampled_columns

MAXLEN = 65535
STEP = DIAGONAL_GAP + K - 1                   # from one diagonal to the next
FOLD_TINY, WALK_MAX, FOLD_SMALL, FOLD_MID, FOLD_LDS, FOLD_SERIAL = 16, 96, 1024, 2048, 4096, 32768
GROUP_PAIRS, GROUP_CHUNK, GROUP_ROUND = 1536, 2048, 8192
FOLD_GRID = 16384                             # workgroups of the short-list instance (bella_hip.hip: wide_batch_finish)
ROUTES = ("tiny", "walk", "grid-partial", "grid", "unstaged", "serial")


def fold_route(m: int, ndiag: int = 1) -> dict:
    """route: what folds a PLAIN chain of m products -- tiny: m <= kWideFoldTiny, k_wide_desc hands the pair to the one-lane fold;
    walk: up to kGridMin, the 16-wide walk over the staged list; grid: the position grid with all of the instance's buckets;
    grid-partial: NB < kGridBuckets (the short-list instance starts at 256 buckets and stops at 8 per product: m <= 128), the only
    lengths on the scan's non-vector branch; unstaged: above 4,096, walk and parent links read HBM; serial: >= 32,768, the parent
    links are u16.  A chain with ndiag > 1 is not plain: the same staging, parents + ancestor walks instead of grid / walk.
    instance: the k_wide_fold_wg instance (None: the pair never reaches one).  redo: more than 16 roots, handed to the one-lane fold."""
    if m <= FOLD_TINY:
        return dict(route="tiny", instance=None, plain=ndiag == 1, redo=False)
    inst = 0 if m <= FOLD_SMALL else 1 if m <= FOLD_MID else 2
    if m >= FOLD_SERIAL:
        return dict(route="serial", instance=inst, plain=ndiag == 1, redo=False)
    if m <= WALK_MAX:
        route = "walk"
    elif m <= FOLD_LDS:
        nb, full = (256, 2048) if inst == 0 else (512, 4096)
        while nb < 8 * m and nb < full:
            nb <<= 1
        route = "grid" if nb == full else "grid-partial"
    else:
        route = "unstaged"
    return dict(route=route, instance=inst, plain=ndiag == 1, redo=ndiag > 16)


class P:
    """a designed pair: m products, layout dense / sparse, ndiag diagonals, rc (None: drawn)"""

    def __init__(self, m, layout="dense", ndiag=1, rc=None):
        assert m >= ndiag >= 1 and (layout == "dense" or ndiag == 1)
        self.m, self.layout, self.ndiag, self.rc = m, layout, ndiag, rc
        self.col = self.partner = None


class Hub:
    def __init__(self, name, pairs):
        self.name, self.ps = name, list(pairs)
        self.F, self.d = sum(p.m for p in self.ps), len(self.ps)
        self.col = None


class WideSet:
    """reads, explicit tuples and the design: hubs, pairs {column: {partner: products}} of EVERY column that has products, and
    specs [P] with col / partner filled in"""

    def stats(self) -> dict:
        return {c: (sum(p.values()), len(p)) for c, p in self.pairs.items()}


def _rand(rng, n):
    return synth.BASES[rng.integers(0, 4, size=n, dtype=np.uint8)]


def _revcomp(s):
    return _COMP[s[::-1]]


class _Builder:
    """collects hubs and partners by index; _finish() gives them read ids (hubs small and unsampled, partners behind them in shuffled
    order) and sorts the tuples"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.hub_seqs, self.part_seqs = [], []
        self.tk, self.tr, self.tp = [], [], []          # tr: hub index h as -1 - h, partner index as is
        self.nkmers = 0
        self.hubs, self.specs, self.part_of = [], [], []  # part_of[partner] = (hub index, P)

    def hub(self, hub, seq, pos):
        """the hub read and the positions of its k-mers (any order) -> their ids, a random permutation"""
        assert len(seq) <= MAXLEN and int(pos.max()) + K <= len(seq)
        h = len(self.hubs)
        ids = self.nkmers + self.rng.permutation(len(pos))
        self.nkmers += len(pos)
        self.hubs.append(hub)
        self.hub_seqs.append(seq.tobytes())
        self.tk.append(ids); self.tr.append(np.full(len(pos), -1 - h)); self.tp.append(pos)
        return h, ids

    def partner(self, h, p, ids, seq, pos, rc):
        assert len(seq) <= MAXLEN and len(ids) == len(pos) == p.m
        if rc:
            seq, pos = _revcomp(seq), len(seq) - K - pos
        r = len(self.part_seqs)
        self.part_seqs.append(seq.tobytes())
        self.part_of.append((h, p))
        self.tk.append(ids); self.tr.append(np.full(len(pos), r)); self.tp.append(pos)

    def planted(self, hub):
        """a hub whose pairs are laid out one after the other behind its left flank, and their partners"""
        rng = self.rng
        maxd = max(p.ndiag for p in hub.ps)
        flank = 2 * SPACER + STEP * (maxd - 1)
        offs, at = [], 0
        for p in hub.ps:
            span = p.m if p.layout == "dense" else min(12 * p.m, MAXLEN - 2 * SPACER - (K - 1) - flank + SPACER)
            o = np.arange(p.m) if p.layout == "dense" else np.sort(rng.choice(span, p.m, replace=False))
            offs.append(at + o)
            at += span
        length = flank + at + K - 1 + SPACER
        seq = _rand(rng, length)
        h, ids = self.hub(hub, seq, flank + np.concatenate(offs))
        n0 = 0
        for p, o in zip(hub.ps, offs):
            chunks, ppos, at = [_rand(rng, SPACER)], [], SPACER
            for d, part in enumerate(np.array_split(o, p.ndiag)):
                if d:
                    chunks.append(_rand(rng, DIAGONAL_GAP))
                    at += DIAGONAL_GAP
                a, b = int(part[0]), int(part[-1])
                chunks.append(seq[flank + a:flank + b + K])
                ppos.append(at + part - a)
                at += b - a + K
            # one diagonal: the estimate is the same along it whatever the flanks; several: the partner outlasts the hub
            chunks.append(_rand(rng, SPACER if p.ndiag == 1 else length - flank - int(o[0]) + SPACER))
            p.rc = bool(rng.random() < 0.5) if p.rc is None else p.rc
            self.partner(h, p, ids[n0:n0 + p.m], np.concatenate(chunks), np.concatenate(ppos), p.rc)
            n0 += p.m


def _finish(b: _Builder) -> WideSet:
    rng = b.rng
    nh, npart = len(b.hub_seqs), len(b.part_seqs)
    head = 2 * nh + 2
    nreads = max(head + npart, 1024)
    while True:                                               # (the sampled ids depend on the number of reads)
        sampled = sampled_columns(nreads)
        free = np.setdiff1d(np.arange(1, nreads), np.fromiter(sampled, np.int64))
        if len(free) and nh - 1 <= np.searchsorted(free, head):
            break
        head += 64
        nreads = max(head + npart, 1024)
    hcol = np.concatenate([[0], free[:nh - 1]]).astype(np.int64)   # hubs[0] is the ballast: column 0, which is sampled
    assert 0 in sampled and (nh == 1 or hcol[-1] < head)
    pid = head + rng.permutation(npart)
    seqs = [None] * nreads
    for c, s in zip(hcol.tolist(), b.hub_seqs):
        seqs[c] = s
    for r, s in zip(pid.tolist(), b.part_seqs):
        seqs[r] = s
    empty = [r for r in range(nreads) if seqs[r] is None]
    fill = _rand(rng, 2 * SPACER * len(empty)).reshape(len(empty), 2 * SPACER)      # fillers: share nothing
    for r, row in zip(empty, fill):
        seqs[r] = row.tobytes()
    tk, tr, tp = (np.concatenate(x).astype(np.int64) for x in (b.tk, b.tr, b.tp))
    tr = np.where(tr < 0, hcol[np.maximum(-1 - tr, 0)], pid[np.maximum(tr, 0)])
    assert int(tp.max()) <= MAXLEN - K and int(tp.min()) >= 0
    order = np.lexsort((tp, tr))
    t = WideSet()
    t.seqs, t.rs, t.nkmers = seqs, synth.readset_from_seqs(seqs), b.nkmers
    t.tk, t.tr, t.tp = tk[order].astype(np.uint32), tr[order].astype(np.uint32), tp[order].astype(np.uint16)
    t.sampled = sampled
    t.ballast, t.hubs = b.hubs[0], b.hubs[1:]
    for hub, c in zip(b.hubs, hcol.tolist()):
        hub.col = c
    t.pairs = {hub.col: {} for hub in b.hubs}
    t.specs = []
    for r, (h, p) in zip(pid.tolist(), b.part_of):
        p.col, p.partner = b.hubs[h].col, r
        t.pairs[p.col][r] = p.m
        t.specs.append(p)
    # the sample sees the ballast column alone: quarter tables, not a long-list input, no row lists on their own
    assert not any(hub.col in sampled for hub in t.hubs) and all(min(t.pairs[hub.col]) > hub.col for hub in b.hubs)
    got = regime_of(nreads, t.stats())
    assert not got["half_tables"] and not got["long_lists"] and got["ratio1024"] == 128, got
    return t


def build(hubs, seed: int) -> WideSet:
    b = _Builder(seed)
    for hub in [Hub("ballast", [P(8) for _ in range(10)])] + list(hubs):
        b.planted(hub)
    return _finish(b)


# ---- the sets ---------------------------------------------------------------------------------------------------------------------
FOLD_M = (1, 16, 17, 96, 97, 128, 129, 1024, 1025, 2048, 2049, 4096, 4097)
FOLD_SHORT = (1, 16, 17, 96, 97)              # a hub of fewer than 65 products would run in the 64-product LDS tier: one shared hub
FOLD_TWO = (17, 97, 128, 1024, 1025, 2049, 4097)
FOLD_MANY = (600, 1500, 3000, 5000)           # 16 roots stay in the workgroup fold, 17 go to the redo list: all instances and unstaged


def fold_set() -> WideSet:
    """one pair per hub except the shared hubs of the short lists (dense, sparse and two-diagonal forms); 32,767 / 32,768 dense"""
    hubs = []
    for layout in ("dense", "sparse"):
        hubs.append(Hub("short-" + layout, [P(m, layout) for m in FOLD_SHORT]))
        hubs += [Hub("%s-%d" % (layout, m), [P(m, layout)]) for m in FOLD_M if m not in FOLD_SHORT]
    hubs.append(Hub("short-two", [P(16, ndiag=2), P(17, ndiag=2), P(40)]))
    hubs += [Hub("two-%d" % m, [P(m, ndiag=2)]) for m in FOLD_TWO if m != 17]
    hubs += [Hub("%d-diagonals-%d" % (D, m), [P(m, ndiag=D)]) for m in FOLD_MANY for D in (16, 17)]
    hubs += [Hub("dense-%d" % m, [P(m)]) for m in (FOLD_SERIAL - 1, FOLD_SERIAL)]
    return build(hubs, seed=41)


LONG_EDGES = (4096, 8192, 16384, 32768, 49152)
LONG_CLUSTER = 300
_LONG_CUT = (20000, 40000)                    # two diagonals: the hub's part between the cuts stands STEP earlier in the partner


def _long_positions():
    """the clusters and their mirror images (pos -> len - k - pos): a reverse-complemented partner has them at the same places"""
    last = MAXLEN - K
    cl = [np.arange(LONG_CLUSTER)]
    cl += [np.arange(c - LONG_CLUSTER // 2, c + LONG_CLUSTER // 2) for c in LONG_EDGES]     # below and above, no gap between them
    pos = np.concatenate(cl)
    return np.unique(np.concatenate([pos, last - pos]))


LONG_M = (1000, 1500, len(_long_positions()))     # (the last: all 2,751)


def long_read_set() -> WideSet:
    """hubs and partners of 65,535 bases; the products stand in clusters at position 0, on both sides of 4,096, 8,192, 16,384,
    32,768 and 49,152 (the grid's bucket range wraps there, positions 4 NB apart share a bucket), at the last position and at the
    mirror images of all of these (a reverse-complemented partner then has them at the same places): 2,751 positions, thinned to
    m = 1,000 and 1,500 (one pair per fold instance); positions 0, len - k and the k on either side of an edge always kept.
    One diagonal: the partner IS the hub (or its reverse complement).  Two: both reads keep their ends -- hub A | x | B | C, partner
    A | B | x' | C with 716 random bases x, x': A and C on diagonal 0, B (the clusters around 32,768) on diagonal 716; with equal
    lengths the estimate is len - |diagonal| + k, so the pair has two bins (and len + k = 65,552 wraps in the u16 estimate, as it
    does in the reference)."""
    b = _Builder(43)
    b.planted(Hub("ballast", [P(8) for _ in range(10)]))
    allpos = _long_positions()
    lo, hi = _LONG_CUT
    for ndiag in (1, 2):
        for m in LONG_M:
            for rc in (False, True):
                keep = (allpos == 0) | (allpos == MAXLEN - K)                  # thinning spares both ends and k positions on either
                for c in LONG_EDGES:                                          # side of every edge, in both reads' coordinates
                    for x in (allpos, MAXLEN - K - allpos):
                        keep |= (x >= c - K) & (x < c + K)
                pos = np.sort(np.concatenate([allpos[keep], b.rng.choice(allpos[~keep], m - int(keep.sum()), replace=False)]))
                p = P(m, "clusters", 1, rc)
                p.ndiag = ndiag
                seq = _rand(b.rng, MAXLEN)
                h, ids = b.hub(Hub("long-%d-%d-%s" % (ndiag, m, "rc" if rc else "fw"), [p]), seq, pos)
                if ndiag == 1:
                    pseq, ppos = seq.copy(), pos.copy()
                else:
                    assert not ((pos + K > lo) & (pos < lo + STEP)).any() and not ((pos + K > hi) & (pos < hi)).any()
                    pseq = np.concatenate([seq[:lo], seq[lo + STEP:hi], _rand(b.rng, STEP), seq[hi:]])
                    ppos = np.where((pos >= lo + STEP) & (pos < hi), pos - STEP, pos)
                b.partner(h, p, ids, pseq, ppos, rc)
    return _finish(b)


GROUP_F = (65, 2047, 2048, 2049, 8191, 8192, 8193)
OVER_F = 9000                                 # the column of 1,537 partners: with wide_budget = OVER_F it is a batch of its own


def group_set(over: bool) -> WideSet:
    """columns for k_wide_group1 (rounds of 8,192 products) and k_wide_group2_chunks (chunks of 2,048, u16 counters per wavefront
    quarter): F on both sides of a chunk and of a round over 24 pairs of mixed lengths; 4,096 products in ONE pair (every quarter of
    both chunks belongs to it); 1,536 partners -- all the table holds --, 1,400 of them with one product; over: 1,537 partners."""
    rng = np.random.default_rng(47)
    hubs = [Hub("F-%d" % F, [P(m) for m in mults(rng, F, 24, 12)]) for F in GROUP_F]
    hubs.append(Hub("one-pair", [P(2 * GROUP_CHUNK)]))
    hubs.append(Hub("full-table", [P(m) for m in mults(rng, 2300, GROUP_PAIRS, GROUP_PAIRS - 1400)]))
    if over:
        hubs.append(Hub("over", [P(m) for m in mults(rng, OVER_F, GROUP_PAIRS + 1, GROUP_PAIRS + 1 - 1400)]))
    return build(hubs, seed=53 + int(over))


MANY_M, MANY_PER_HUB = 17, 4                  # 68 products per column: above the 64-product tier


def many_pairs_set(pairs: int = 8 * FOLD_GRID + 8) -> WideSet:
    """pairs of 17 products (the shortest list that gets a workgroup), four to a column: with more than 8 x 16,384 of them a workgroup
    of the short-list instance folds more than eight pairs -- it loops, prefetches two ahead and flushes its eight pending records
    inside the loop.  Built vectorised: every hub is its four stretches and a tail, every partner spacer + stretch + spacer."""
    assert pairs % MANY_PER_HUB == 0
    b = _Builder(59)
    b.planted(Hub("ballast", [P(8) for _ in range(10)]))
    rng, nh, m = b.rng, pairs // MANY_PER_HUB, MANY_M
    nk = m * MANY_PER_HUB
    hseq = _rand(rng, nh * (nk + K - 1)).reshape(nh, nk + K - 1)
    win = np.arange(m + K - 1)
    st = hseq[:, (m * np.arange(MANY_PER_HUB))[:, None] + win].reshape(pairs, m + K - 1)       # the stretch of every pair
    rc = rng.random(pairs) < 0.5
    st = np.where(rc[:, None], _COMP[st[:, ::-1]], st)
    pseq = np.concatenate([_rand(rng, pairs * SPACER).reshape(pairs, SPACER), st, _rand(rng, pairs * SPACER).reshape(pairs, SPACER)], axis=1)
    ids = b.nkmers + np.argsort(rng.random((nh, nk)), axis=1) + nk * np.arange(nh)[:, None]      # a permutation per hub
    b.nkmers += nh * nk
    h0, r0 = len(b.hubs), len(b.part_seqs)
    hubs = [Hub("h", []) for _ in range(nh)]
    specs = [P(m, rc=bool(x)) for x in rc.tolist()]
    for h, hub in enumerate(hubs):
        hub.ps = specs[MANY_PER_HUB * h:MANY_PER_HUB * (h + 1)]
        hub.F, hub.d = nk, MANY_PER_HUB
    b.hubs += hubs
    b.hub_seqs += [row.tobytes() for row in hseq]
    b.part_seqs += [row.tobytes() for row in pseq]
    b.part_of += [(h0 + x // MANY_PER_HUB, p) for x, p in enumerate(specs)]
    b.tk += [ids.ravel(), ids.ravel()]
    b.tr += [np.repeat(-1 - h0 - np.arange(nh), nk), np.repeat(r0 + np.arange(pairs), m)]
    j = np.arange(m)
    b.tp += [np.tile(np.arange(nk), nh), (SPACER + np.where(rc[:, None], m - 1 - j, j)).ravel()]
    return _finish(b)
