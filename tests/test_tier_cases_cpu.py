"""The sets of bella_testkit/tier_cases.py have the columns they are for: the oracle finds in every hub column exactly the designed
products, pairs and products per pair, and no product anywhere else -- so that a failure of tests/test_row_tiers_gpu.py on these
sets is a failure of the kernels.  The oracle's `count` field is the reference's chain count, not a pair's products; the products per
pair are counted here from the oracle's own B and its transpose."""
import numpy as np
import pytest

import _oracle as O
from bella_testkit import tier_cases as T

CASES = [(r, c) for r in "QH" for c in (T.CAPS[r][0], T.CAPS[r][len(T.CAPS[r]) // 2], T.CAPS[r][-1])]


def oracle_columns(t):
    """-> flop, pairs per column, {column: {partner: products}} from B and A = B^T, records"""
    nr = t.rs.nreads
    Bc, Br, Bv = O.build_B(nr, t.tk, t.tr, t.tp)
    flop, colptrC, recs = O.spgemm(t.seqs, t.nkmers, Bc, Br, Bv, T.K)
    Ac, Ar, _ = O.transpose(nr, t.nkmers, Bc, Br, Bv)
    col = np.repeat(np.arange(nr), np.diff(Bc.astype(np.int64)))            # column of every B entry
    n = np.diff(Ac.astype(np.int64))[Br]                                    # reads that hold its k-mer
    e = np.repeat(np.arange(len(Br)), n)
    partner = Ar[np.repeat(Ac[:-1].astype(np.int64)[Br], n) + np.arange(len(e)) - np.repeat(np.cumsum(n) - n, n)]
    keep = partner > col[e]
    key, cnt = np.unique(col[e][keep].astype(np.int64) * nr + partner[keep], return_counts=True)
    per = {}
    for kk, c in zip(key.tolist(), cnt.tolist()):
        per.setdefault(kk // nr, {})[kk % nr] = c
    return np.asarray(flop).astype(np.int64), np.diff(colptrC.astype(np.int64)), per, recs


def check_design(t):
    flop, npairs, per, recs = oracle_columns(t)
    st = t.stats()
    want_f = np.zeros(t.rs.nreads, np.int64)
    want_d = np.zeros(t.rs.nreads, np.int64)
    for c, (F, d) in st.items():
        want_f[c], want_d[c] = F, d
    assert np.array_equal(flop, want_f)                                     # every hub as designed, no product in any other column
    assert np.array_equal(npairs, want_d)
    assert per == t.pairs
    assert int(recs["count"].max()) > 1
    return flop


@pytest.mark.parametrize("regime,cap", CASES)
def test_edge_set_has_the_columns_it_is_for(regime, cap):
    t = T.edge_set(cap, regime)
    check_design(t)
    C, D = cap, T.dcap_of(cap, regime)
    Mc = T.mcap_of(D)
    assert D == {"Q": C // 4, "H": C if C <= 300 else C // 2 if C <= 4096 else C // 4}[regime]
    by = {h.name: h for h in t.hubs}
    h = by["full-dense"]
    assert (h.F, h.d, h.nm) == (C, D, min(Mc, C - D))
    if D < C:                                                               # a table as large as the tier leaves no pair a second product
        assert by["full-dense"].nm == Mc
        h = by["full-slot-scan"]
        assert (h.F, h.d, h.nm) == (C, D, Mc + 1)
        h = by["overflow"]
        assert (h.F, h.d, h.nm) == (C, D + 1, Mc)
    else:
        assert "full-slot-scan" not in by and "overflow" not in by
    h = by["above"]
    assert (h.F, h.d) == (C + 1, D) and h.nm <= Mc
    h = by["below-all-multi"]
    assert (h.F, h.d) == (C - 1, min(D, (C - 1) // 2)) and h.nm == h.d and min(h.mults) >= 2
    h = by["one-pair"]
    assert (h.F, h.d, h.mults) == (C, 1, [C])
    h = by["shared"]
    assert h.F == C // 2 and h.d <= D
    later = np.unique(t.tk, return_counts=True)[1] - 1                      # hub entries with two and three later reads
    assert (later == 2).any() and (later == 3).any()
    same = t.tr[1:] == t.tr[:-1]                                            # tuples are in (read, position) order
    gap = np.diff(t.tp.astype(np.int64))[same] > 500                        # the pair on two diagonals: its stretches are 700 bases apart
    assert int(gap.sum()) == 1 and int(t.tr[1:][same][gap][0]) in t.pairs[h.col]
    step = np.diff(t.tk.astype(np.int64))[same]                             # both strands: k-mers ascending and descending along partners
    assert (step == 1).any() and (step == -1).any()
    for F in (255, 256, 257):
        assert by["ragged-%d" % F].F == F and by["ragged-%d" % F].d <= D
    assert t.retries(C, D) == (1 if D < C else 0)
    # the regime: no hub on a sampled column in Q; the sample restated from the oracle's own numbers
    if regime == "Q":
        assert t.rs.nreads >= 1024 and not any(h.col in t.sampled for h in t.hubs) and t.ballast.col in t.sampled
    assert t.sampled == T.sampled_columns(t.rs.nreads)
    flop, npairs, _, _ = oracle_columns(t)
    got = T.regime_of(t.rs.nreads, {c: (int(flop[c]), int(npairs[c])) for c in np.flatnonzero(flop)})
    assert got["half_tables"] == (regime == "H") and not got["long_lists"]


@pytest.mark.parametrize("regime", ["Q", "H"])
def test_table_and_small_class_sets(regime):
    t = T.table_set(regime)
    check_design(t)
    caps = T.TABLE[regime]
    have = {h.F: h.d for h in t.hubs}
    for C in caps:
        for F in (C - 1, C, C + 1):
            own = min([c for c in caps if c >= F], default=caps[-1])
            assert have[F] == min(T.dcap_of(own, regime), F)
    for F, d in t.stats().values():                                         # no column has more pairs than its own tier's table holds
        assert F > caps[-1] or d <= T.dcap_of(min(c for c in caps if c >= F), regime)
    s = T.small_class_set(regime)
    check_design(s)
    fs = {h.F for h in s.hubs}
    assert fs == set(T.SMALL_CLASS_TIERS) - set(T.SMALL_CLASS_EMPTY)
    assert max(h.d for h in s.hubs) == min(T.dcap_of(192, regime), 192)


def test_top_edge_sets():
    for n, length, f0 in ((16, 4385, 65535), (17, 4112, 65536)):
        t = T.top_edge_set(n, length)
        flop = check_design(t)
        nk = length - T.K + 1
        assert len(t.same_cols) == n and len({t.seqs[c] for c in t.same_cols}) == 1
        assert [int(flop[c]) for c in t.same_cols] == [nk * (n - 1 - x) for x in range(n)] and int(flop[t.same_cols[0]]) == f0
        assert int(flop.max()) == f0
        assert int(((flop > 11008) & (flop <= 65535)).sum()) == 13            # fewer than 16: the global-workspace path
        # the sample sees the ballast column alone: quarter tables, every default tier open, no row lists on their own
        assert t.rs.nreads >= 1024 and not any(c in t.sampled for c in t.same_cols) and t.ballast.col in t.sampled
        npairs = oracle_columns(t)[1]
        got = T.regime_of(t.rs.nreads, {c: (int(flop[c]), int(npairs[c])) for c in np.flatnonzero(flop)})
        assert not got["half_tables"] and not got["long_lists"] and got["ratio1024"] == 128
