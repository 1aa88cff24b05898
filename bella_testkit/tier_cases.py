"""Read sets whose columns sit on the edges of the row kernels' LDS tiers (bella_hip.hip: kTierCapsDefault / kTierCapsHalf, dcap_of;
spgemm.hpp: process_row).  Test tooling: nothing here is used by the product.

A column is built for its product count F, its pair count d and the products of every pair:
    a HUB is a random read of n + k - 1 bases; its n consecutive k-mers are its B' entries;
    a PARTNER carries, between random 20-base spacers, the stretch hub[off : off + m + k - 1] -- m consecutive k-mers of the hub, one
    pair with m products -- and the next partner starts at off + m.  About half of the stretches are planted as their reverse
    complement, the positions mirrored.  A stretch given to s partners makes hub entries with s later reads (and products among those
    partners, which the design lists too); a partner with two stretches 700 bases apart is a pair on two diagonals.
Hubs get small read ids, partners larger ones in shuffled order, so a hub's column pairs with its partners and the order of the key
table's slots is not the order of the products.  The k-mers are handed over as explicit tuples (kmer, read, pos): counting k-mers
would add the chance collisions of random 17-mers (at 2,700 reads: one hub off by two products at cap 11,008).

The regime -- which key-table budget a pass runs with -- follows from k_sample_pair_ratio (spgemm.hpp), restated in regime_of():
it looks at the columns j * step, step = (nreads + 1) // min(nreads + 1, 512), and ignores columns with fewer than 64 products.
    Q   quarter-size key tables: at least 1,024 reads (short filler reads that share nothing), every hub on an id that is not
        sampled, one sampled ballast column of 80 products over 10 pairs (ratio 128 / 1024);
    H   half-size tables: one sampled ballast column of 256 products over 256 pairs (ratio 1024 / 1024)."""
from __future__ import annotations

import numpy as np

from . import synth

K = 17
SPACER = 20
DIAGONAL_GAP = 700                         # > binSize (500): the second stretch of the two-diagonal pair opens another overlap bin
CAPS = {"Q": (384, 689, 1000, 1394, 2048, 2752, 3712, 4600, 5568, 8192, 11008),            # the LDS tiers of kTierCapsDefault
        "H": (300, 526, 800, 1064, 1600, 2105, 2789, 3500, 4096, 6144)}                    # ... of kTierCapsHalf, single-tier runs
TABLE = {"Q": CAPS["Q"], "H": CAPS["H"] + (8192, 11008)}                                   # every LDS tier of the default tables
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def dcap_of(cap: int, regime: str) -> int:
    """pairs the key table of a tier holds (bella_hip.hip: dcap_of; kFullTableMaxCap = 300, kHalfTableMaxCap = 4096)"""
    if regime == "H" and cap <= 300:
        return cap
    if regime == "H" and cap <= 4096:
        return cap // 2
    return cap // 4


def mcap_of(dcap: int) -> int:
    """entries of the dense list M of multi-product pairs (spgemm.hpp: Mcap)"""
    return (dcap + 1) // 2


def sampled_columns(nreads: int) -> set:
    ncols = nreads + 1
    nsample = min(ncols, 512)
    step = max(ncols // nsample, 1)
    return {j * step for j in range(nsample) if j * step < nreads}


def regime_of(nreads: int, columns: dict) -> dict:
    """columns: {column: (F, d)} of every column with products -> what the assembly-time sample makes of them"""
    ratio, pairs, p64 = 0, 0, 0
    for c in sampled_columns(nreads):
        F, d = columns.get(c, (0, 0))
        if F >= 64:
            ratio = max(ratio, (d << 10) // F)
        pairs += d
        p64 += min(F >> 6, 1 << 20)
    return dict(ratio1024=ratio, half_tables=ratio * 5 >= 1024, long_lists=ratio < 16 or (p64 > 0 and pairs <= p64))


def mults(rng, F: int, d: int, nm: int) -> list:
    """the products of d pairs, nm of them with two or more, F in all, in shuffled order"""
    assert 0 < d and nm <= d and d + nm <= F and (nm > 0 or F == d), (F, d, nm)
    m = np.ones(d, np.int64)
    m[:nm] = 2
    if F - d - nm:
        m[:nm] += rng.multinomial(F - d - nm, np.full(nm, 1.0 / nm))
    rng.shuffle(m)
    return [int(x) for x in m]


def plain(ms) -> list:
    """groups of a hub whose every stretch goes to one partner"""
    return [((m,), 1) for m in ms]


class Hub:
    """name, groups [((stretch lengths), partners that get them)] -> the designed F, d and products per pair"""

    def __init__(self, name, groups):
        self.name, self.groups = name, groups
        self.nk = sum(sum(lens) for lens, _ in groups)
        self.mults = sorted(sum(lens) for lens, share in groups for _ in range(share))
        self.F, self.d = sum(self.mults), len(self.mults)
        self.nm = sum(1 for m in self.mults if m > 1)
        self.col = None


class TierSet:
    """reads, explicit tuples, and the design: hubs (list of Hub, column ids filled in) and pairs {column: {partner: products}} of
    EVERY column that has products"""

    def stats(self) -> dict:
        return {c: (sum(p.values()), len(p)) for c, p in self.pairs.items()}

    def retries(self, cap: int, dcap: int) -> int:
        """columns of an LDS tier of `cap` products whose pairs do not fit a key table of `dcap` slots"""
        return sum(1 for F, d in self.stats().values() if F <= cap and d > dcap)


def _random_bases(rng, n):
    return synth.BASES[rng.integers(0, 4, size=n, dtype=np.uint8)]


def _partners(hubs) -> list:
    """(hub index, group index, [(first hub k-mer, k-mers)]) of every partner, in product order"""
    parts = []
    for h, hub in enumerate(hubs):
        off = 0
        for g, (lens, share) in enumerate(hub.groups):
            segs = []
            for m in lens:
                segs.append((off, m))
                off += m
            parts += [(h, g, segs)] * share
    return parts


def _assign_ids(hubs, same: int, nparts: int, regime: str, rng):
    """-> reads of the set, its sampled columns, the columns of the `same` identical reads, the partners' ids.  hubs[0] (the ballast)
    takes column 0, which is sampled; in Q every other hub and every identical read steps over the sampled ids.  Partner ids follow
    the head in shuffled order: not the product order."""
    head = 2 * (len(hubs) + same) + 2
    nreads = max(head + nparts, 1024 if regime == "Q" else 0)
    sampled = sampled_columns(nreads)
    assert 0 in sampled
    cols, col = [], 0
    for n in range(len(hubs) + same):
        if n and regime == "Q":
            while col in sampled:
                col += 1
        cols.append(col)
        col += 1
    assert col <= head
    for hub, c in zip(hubs, cols):
        hub.col = c
    return nreads, sampled, cols[len(hubs):], head + rng.permutation(nparts)


def _lay_out(hubs, parts, pid, nreads: int, rng):
    """-> sequences (None where no read was laid out), tuples (kmer, read, pos), k-mers"""
    seqs = [None] * nreads
    base = np.concatenate([[0], np.cumsum([hub.nk for hub in hubs])])
    hubseq, tk, tr, tp = [], [], [], []
    for h, hub in enumerate(hubs):
        s = _random_bases(rng, hub.nk + K - 1)
        hubseq.append(s)
        seqs[hub.col] = s.tobytes()
        tk.append(base[h] + np.arange(hub.nk))
        tr.append(np.full(hub.nk, hub.col))
        tp.append(np.arange(hub.nk))
    for (h, g, segs), r in zip(parts, pid):
        chunks, pos = [_random_bases(rng, SPACER)], SPACER
        for n, (off, m) in enumerate(segs):
            if n:
                chunks.append(_random_bases(rng, DIAGONAL_GAP))
                pos += DIAGONAL_GAP
            st = hubseq[h][off:off + m + K - 1]
            j = np.arange(m)
            if rng.random() < 0.5:                                # the other strand: k-mer off + j sits at mirrored position m - 1 - j
                st = _COMP[st[::-1]]
                j = m - 1 - j
            chunks.append(st)
            tk.append(base[h] + off + np.arange(m))
            tr.append(np.full(m, int(r)))
            tp.append(pos + j)
            pos += m + K - 1
        chunks.append(_random_bases(rng, SPACER))
        seqs[int(r)] = np.concatenate(chunks).tobytes()
    return seqs, [tk, tr, tp], int(base[-1])


def _lay_out_same(cols, length: int, first_kmer: int, seqs, tuples, rng) -> int:
    """one random read of `length` bases on every column of `cols`, every k-mer in all of them -> k-mers added"""
    nk = length - K + 1
    s = _random_bases(rng, length).tobytes()
    for c in cols:
        seqs[c] = s
        tuples[0].append(first_kmer + np.arange(nk))
        tuples[1].append(np.full(nk, c))
        tuples[2].append(np.arange(nk))
    return nk


def _design(hubs, parts, pid) -> dict:
    """{column: {partner: products}}: a hub with each of its partners, and the partners that got the same stretch among themselves"""
    pairs = {hub.col: {} for hub in hubs}
    groups = {}
    for (h, g, segs), r in zip(parts, pid):
        pairs[hubs[h].col][int(r)] = sum(m for _, m in segs)
        groups.setdefault((h, g), []).append(int(r))
    for (h, g), ids in groups.items():
        ids.sort()
        m = sum(hubs[h].groups[g][0])
        for x, a in enumerate(ids):
            for b in ids[x + 1:]:
                pairs.setdefault(a, {})[b] = m
    return pairs


def build(hubs, regime: str, seed: int = 0, same=(0, 0)) -> TierSet:
    """the set of `hubs` plus the regime's ballast column; same = (n, length): n identical reads of `length` bases as well"""
    rng = np.random.default_rng(seed)
    ballast = Hub("ballast", plain([8] * 10) if regime == "Q" else plain([1] * 256))
    hubs = [ballast] + list(hubs)
    parts = _partners(hubs)
    nreads, sampled, same_cols, pid = _assign_ids(hubs, same[0], len(parts), regime, rng)
    seqs, tuples, nkmers = _lay_out(hubs, parts, pid, nreads, rng)
    pairs = _design(hubs, parts, pid)
    if same_cols:
        nk = _lay_out_same(same_cols, same[1], nkmers, seqs, tuples, rng)
        nkmers += nk
        for x, c in enumerate(same_cols[:-1]):
            pairs[c] = {r: nk for r in same_cols[x + 1:]}
    for r in range(nreads):
        if seqs[r] is None:
            seqs[r] = _random_bases(rng, 2 * SPACER).tobytes()      # filler: shares nothing
    tk, tr, tp = (np.concatenate(x) for x in tuples)
    assert int(tp.max()) < 65536
    order = np.lexsort((tp, tr))
    t = TierSet()
    t.regime, t.hubs, t.ballast, t.pairs, t.same_cols = regime, hubs[1:], ballast, pairs, same_cols
    t.seqs = seqs
    t.rs = synth.readset_from_seqs(seqs)
    t.nkmers = nkmers
    t.tk, t.tr, t.tp = tk[order].astype(np.uint32), tr[order].astype(np.uint32), tp[order].astype(np.uint16)
    t.sampled = sampled
    _check(t)
    return t


def _check(t: TierSet) -> None:
    """the design holds what the hubs were specified with, and the sample sees the regime the set is for"""
    for hub in [t.ballast] + t.hubs:
        own = t.pairs[hub.col]
        assert own and sum(own.values()) == hub.F and len(own) == hub.d
        assert sorted(own.values()) == hub.mults and min(own) > hub.col
    if t.regime == "Q":
        assert not any(c in t.sampled for c in [hub.col for hub in t.hubs] + t.same_cols)
    got = regime_of(t.rs.nreads, t.stats())
    assert got["half_tables"] == (t.regime == "H") and not got["long_lists"], got


def edge_hubs(cap: int, regime: str, rng) -> list:
    """the hubs of one tier (C = cap, D = its key table, Mc = its dense list).  Where the table is as large as the tier (H, cap <= 300)
    a column with D pairs has no product left for a second one in any pair: the dense list cannot fill, the slot-scan hub does not
    exist and neither does the overflow (D + 1 pairs need D + 1 products)."""
    C, D = cap, dcap_of(cap, regime)
    Mc = mcap_of(D)
    hubs = [Hub("full-dense", plain(mults(rng, C, D, min(Mc, C - D))))]
    if D + Mc + 1 <= C:
        hubs.append(Hub("full-slot-scan", plain(mults(rng, C, D, Mc + 1))))
    if D + 1 <= C:
        hubs.append(Hub("overflow", plain(mults(rng, C, D + 1, min(Mc, C - D - 1)))))
    hubs.append(Hub("above", plain(mults(rng, C + 1, D, min(Mc, C + 1 - D)))))
    d = min(D, (C - 1) // 2)
    hubs.append(Hub("below-all-multi", plain(mults(rng, C - 1, d, d))))
    hubs.append(Hub("one-pair", plain([C])))
    # entries with two and three later reads, a pair on two diagonals, the rest mixed: C // 2 products
    rest = C // 2 - (2 * 24 + 3 * 16 + 40)
    dr = max(1, min(rest // 3, D - 6))
    hubs.append(Hub("shared", [((24,), 2), ((20, 20), 1), ((16,), 3)] + plain(mults(rng, rest, dr, min(dr // 2, rest - dr)))))
    for F in (255, 256, 257):
        if F <= C:
            d = min(D, F // 3)
            hubs.append(Hub("ragged-%d" % F, plain(mults(rng, F, d, d // 2))))
    return hubs


def edge_set(cap: int, regime: str) -> TierSet:
    """the set of one single-tier run"""
    rng = np.random.default_rng(cap)
    t = build(edge_hubs(cap, regime, rng), regime, seed=cap + 1)
    t.cap, t.dcap = cap, dcap_of(cap, regime)
    return t


def table_set(regime: str) -> TierSet:
    """hubs of C - 1, C and C + 1 products for every LDS tier of the regime's default table, each with as many pairs as the key table
    of its OWN tier holds (11,009 products: above the tiers, 2,752 pairs)"""
    rng = np.random.default_rng(len(regime))
    caps = TABLE[regime]
    hubs = []
    for C in caps:
        for F in (C - 1, C, C + 1):
            own = min([c for c in caps if c >= F], default=caps[-1])
            D = min(dcap_of(own, regime), F)
            hubs.append(Hub("%d" % F, plain(mults(rng, F, D, min(mcap_of(D), F - D)))))
    return build(hubs, regime, seed=7)


SMALL_CLASS_TIERS = (64, 80, 96, 112, 128, 160, 192)
SMALL_CLASS_EMPTY = (80, 128)


def small_class_set(regime: str) -> TierSet:
    """seven tiers in the smallest class (the launch reads their counts from the control block): hubs at every cap but two, with the
    pairs the class's key table (that of its largest tier) holds"""
    rng = np.random.default_rng(3)
    D = dcap_of(SMALL_CLASS_TIERS[-1], regime)
    hubs = []
    for C in SMALL_CLASS_TIERS:
        if C in SMALL_CLASS_EMPTY:
            continue
        d = min(D, C)
        hubs.append(Hub("%d" % C, plain(mults(rng, C, d, min(mcap_of(d), C - d)))))
        hubs.append(Hub("%d-one-pair" % C, plain([C])))
    return build(hubs, regime, seed=11)


def top_edge_set(nsame: int, length: int) -> TierSet:
    """nsame identical reads of `length` bases, every k-mer in all of them: the first of them has (length - k + 1) * (nsame - 1)
    products.  Built like the Q sets -- 1,024 reads, the identical reads on ids that are not sampled, the sampled ballast column --
    because a sample that saw these columns (15 pairs over 65,535 products) would call the input a long-list one: the larger LDS tiers
    would close and the row lists would be built on their own, whatever operand form was asked for."""
    return build([], "Q", seed=5, same=(nsame, length))
