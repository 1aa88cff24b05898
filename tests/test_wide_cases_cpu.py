"""The sets of bella_testkit/wide_cases.py have the pairs they are for: the oracle finds in every hub column exactly the designed
pairs with exactly their products and no product anywhere else, every pair ends with as many bins as it has diagonals, the sparse
lists make the fold count differently from the dense ones, the long reads carry products at both ends of both reads, the columns
of 1,536 / 1,537 partners have exactly that many, and the sample sees the regime the sets are laid out for -- so that a failure of
tests/test_wide_edges_gpu.py on these sets is a failure of wide.hpp.  The products per pair are counted from the oracle's own B and
its transpose (test_tier_cases_cpu.oracle_columns)."""
import numpy as np
import pytest

import _oracle as O
from bella_testkit import tier_cases as T
from bella_testkit import wide_cases as W
from test_tier_cases_cpu import oracle_columns


def check_design(t):
    """-> {(column, partner): record}"""
    flop, npairs, per, recs = oracle_columns(t)
    want_f = np.zeros(t.rs.nreads, np.int64)
    want_d = np.zeros(t.rs.nreads, np.int64)
    for c, (F, d) in t.stats().items():
        want_f[c], want_d[c] = F, d
    assert np.array_equal(flop, want_f)                                     # every hub as designed, no product in any other column
    assert np.array_equal(npairs, want_d)
    assert per == t.pairs
    for hub in t.hubs:
        assert (int(flop[hub.col]), int(npairs[hub.col])) == (hub.F, hub.d) and hub.F > 64, hub.name
    # the regime, restated from the oracle's own numbers: the sample sees the ballast column alone
    assert t.rs.nreads >= 1024 and t.sampled == T.sampled_columns(t.rs.nreads)
    assert t.ballast.col in t.sampled and not any(h.col in t.sampled for h in t.hubs)
    got = T.regime_of(t.rs.nreads, {c: (int(flop[c]), int(npairs[c])) for c in np.flatnonzero(flop)})
    assert not got["half_tables"] and not got["long_lists"] and got["ratio1024"] == 128
    assert len(recs) == len(t.specs) and len({(p.col, p.partner) for p in t.specs}) == len(recs)
    at = {(int(c), int(r)): n for n, (c, r) in enumerate(zip(recs["cid"].tolist(), recs["rid"].tolist()))}
    nb = np.array([recs["nbins"][at[(p.col, p.partner)]] for p in t.specs])
    assert np.array_equal(nb, [p.ndiag for p in t.specs])                   # one bin per diagonal: every single-diagonal pair has one
    return {key: recs[n] for key, n in at.items()}


def test_fold_route_restates_the_thresholds():
    r = W.fold_route
    assert [r(m)["route"] for m in (1, 16, 17, 96, 97, 128, 129, 4096, 4097, 32767, 32768)] == \
        ["tiny", "tiny", "walk", "walk", "grid-partial", "grid-partial", "grid", "grid", "unstaged", "unstaged", "serial"]
    assert [r(m)["instance"] for m in (16, 17, 1024, 1025, 2048, 2049, 32767)] == [None, 0, 0, 1, 1, 2, 2]
    assert [r(m)["route"] for m in (1025, 2048, 2049)] == ["grid"] * 3      # 512 threads: 4,096 buckets from the first length on
    assert not r(600, 16)["redo"] and r(600, 17)["redo"] and not r(600, 17)["plain"] and r(600)["plain"]


def test_fold_set_has_a_pair_on_every_route():
    t = W.fold_set()
    rec = check_design(t)
    by = {}
    for p in t.specs:
        by.setdefault((p.m, p.layout, p.ndiag), []).append(p)
    for m in W.FOLD_M:
        assert (m, "dense", 1) in by and (m, "sparse", 1) in by
    for m in W.FOLD_TWO:
        assert (m, "dense", 2) in by
    for m in W.FOLD_MANY:
        assert (m, "dense", 16) in by and (m, "dense", 17) in by
    assert (32767, "dense", 1) in by and (32768, "dense", 1) in by
    for key in ("dense", "sparse"):                                         # strands mixed
        assert {p.rc for p in t.specs if p.layout == key and p.m > 8} == {False, True}
    assert {p.rc for p in t.specs if p.ndiag > 1} == {False, True}
    # the sparse lists of the grid's instances count further than the dense ones: the fold did real work
    for m in (1024, 1025, 2048, 2049, 4096, 4097):
        d, s = by[(m, "dense", 1)][0], by[(m, "sparse", 1)][0]
        assert int(rec[(d.col, d.partner)]["count"]) != int(rec[(s.col, s.partner)]["count"]), m
    # ... and wraps mod 2^16: the closed form of a plain chain restated (count = m + for every product the later products before the
    # first one within k of it in either coordinate), in the product order of the oracle's own B
    Bc, Br, _ = O.build_B(t.rs.nreads, t.tk, t.tr, t.tp)
    wrapped = 0
    for m in (2048, 2049, 4096, 4097):
        s = by[(m, "sparse", 1)][0]
        at = {}
        for r in (s.col, s.partner):
            sel = t.tr == r
            at[r] = dict(zip(t.tk[sel].tolist(), t.tp[sel].astype(np.int64).tolist()))
        order = Br[int(Bc[s.col]):int(Bc[s.col + 1])].tolist()
        h, v = (np.array([at[r][kk] for kk in order]) for r in (s.col, s.partner))
        near = (np.abs(h[:, None] - h[None, :]) <= W.K) | (np.abs(v[:, None] - v[None, :]) <= W.K)
        near &= np.arange(m)[None, :] > np.arange(m)[:, None]
        first = np.where(near.any(axis=1), near.argmax(axis=1), m)
        total = m + int((first - np.arange(m) - 1).sum())
        assert int(rec[(s.col, s.partner)]["count"]) == total & 0xFFFF, m
        wrapped += total >= 65536
    assert wrapped >= 2
    # every route plain; every route but the one-lane folds' own (a pair of one diagonal per design there) in non-plain form; the
    # hand-over of more than 16 roots from all three instances and from an unstaged list
    plain, other, redo = set(), set(), set()
    for p in t.specs + t.ballast.ps:
        f = W.fold_route(p.m, p.ndiag)
        (plain if f["plain"] else other).add((f["route"], f["instance"]))
        if f["redo"]:
            redo.add((f["route"], f["instance"]))
    every = {("tiny", None), ("walk", 0), ("grid-partial", 0), ("grid", 0), ("grid", 1), ("grid", 2), ("unstaged", 2), ("serial", 2)}
    assert plain == every
    assert other == every - {("serial", 2)}
    assert redo == {("grid", 0), ("grid", 1), ("grid", 2), ("unstaged", 2)}
    stay = {(W.fold_route(p.m, p.ndiag)["route"], W.fold_route(p.m, p.ndiag)["instance"]) for p in t.specs if p.ndiag == 16}
    assert stay == redo


def test_long_read_set_reaches_both_ends_of_both_reads():
    t = W.long_read_set()
    check_design(t)
    last = W.MAXLEN - W.K
    assert sorted((p.m, p.ndiag, p.rc) for p in t.specs if p.m > 8) == sorted((m, d, rc) for m in W.LONG_M for d in (1, 2) for rc in (False, True))
    for p in t.specs:
        if p.m == 8:
            continue
        for r in (p.col, p.partner):
            assert len(t.seqs[r]) == W.MAXLEN
            pos = t.tp[t.tr == r].astype(np.int64)
            assert len(pos) == p.m and pos.min() == 0 and pos.max() == last
            for c in W.LONG_EDGES:                                          # within k of the edge on both of its sides
                if p.ndiag == 2 and r == p.partner and c == 32768:          # (the part on the second diagonal stands 716 earlier there)
                    continue
                assert ((pos >= c - W.K) & (pos < c)).any() and ((pos >= c) & (pos < c + W.K)).any(), (p.m, c)


@pytest.mark.parametrize("over", [False, True])
def test_group_set_columns(over):
    t = W.group_set(over)
    check_design(t)
    st = {h.name: (h.F, h.d) for h in t.hubs}
    for F in W.GROUP_F:
        assert st["F-%d" % F] == (F, 24)
    assert st["one-pair"] == (2 * W.GROUP_CHUNK, 1)
    assert st["full-table"][1] == W.GROUP_PAIRS == 1536
    assert ("over" in st) == over
    if over:
        assert st["over"] == (W.OVER_F, 1537)
        assert max(F for name, (F, _) in st.items() if name != "over") < W.OVER_F     # a budget of OVER_F: the column is a batch of its own
    singles = sum(1 for p in t.specs if p.col == [h for h in t.hubs if h.name == "full-table"][0].col and p.m == 1)
    assert singles == 1400
    assert max(d for _, d in st.values()) == (1537 if over else 1536)


def test_many_pairs_set():
    t = W.many_pairs_set()
    check_design(t)
    assert len(t.specs) - 10 == 8 * W.FOLD_GRID + 8
    assert all((h.F, h.d) == (68, 4) for h in t.hubs)
    assert {p.m for p in t.specs} == {8, 17}
