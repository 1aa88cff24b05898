"""B' with one entry per product (BELLA_TUNE_PRODUCT_ENTRIES, assemble.hpp: k_layout_compact_products) and the row kernels without an
expansion phase (spgemm.hpp: PE): every path that reads such a layout against the oracle, exactly as test_spgemm_pairs_bit_exact
compares -- products, pair count, colptrC, every record field, the diagnostics array."""
import numpy as np
import pytest

import _oracle as O
from bella_amd import BellaPars, Engine, api
from bella_testkit import synth
from conftest import GOLDEN_SETS, load_golden, set_mode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def oracle_pairs(rs, seqs, nkmers, tk, tr, tp, k=17):
    Bc, Br, Bv = O.build_B(rs.nreads, tk, tr, tp)
    flop, colptrC, pairs = O.spgemm(seqs, nkmers, Bc, Br, Bv, k)
    return (Bc, Br, Bv), flop, colptrC, pairs


def check_pairs(got, ext, exp, lengths, k):
    assert len(got) == len(exp)
    for f in ("rid", "cid", "count", "seedH", "seedV"):
        assert np.array_equal(got[f], exp[f]), f
    for f in ("nbins", "support", "binov"):
        assert np.array_equal(ext[f], exp[f]), f
    assert np.array_equal(api.overlap_of_seed(got, lengths, k), exp["overlap"].astype(np.int64))


class Case:
    """operands + the oracle's answer, computed once and shared"""

    def __init__(self, rs, seqs, k, nkmers, tk, tr, tp):
        self.rs, self.seqs, self.k, self.nkmers, self.tk, self.tr, self.tp = rs, seqs, k, nkmers, tk, tr, tp
        self.B, self.flop, self.ecol, self.exp = oracle_pairs(rs, seqs, nkmers, tk, tr, tp, k)
        self.flop = np.asarray(self.flop).astype(np.int64)
        self.ecnt = np.diff(self.ecol.astype(np.int64))
        for a in (self.flop, self.ecol, self.exp, self.ecnt):
            a.setflags(write=False)

    def pars(self):
        return BellaPars(skipAlignment=True, kmerSize=self.k)


_cases = {}


def golden_case(name):
    if name not in _cases:
        g = load_golden(name)
        _cases[name] = Case(g.rs, g.seqs, g.k, g.nkmers, g.tk, g.tr, g.tp)
    return _cases[name]


def synth_case():
    """300 reads of 1,600 .. 6,400 bases at 10 % error: columns of every size class, chosen on the CPU with the oracle"""
    if "synth" not in _cases:
        rs = synth.make_reads(300, read_len=4000, coverage=30, err=0.10, seed=2, len_jitter=0.6)
        t = synth.count_and_tuples(rs, 17, 2, 8)
        _cases["synth"] = Case(rs, rs.seqs(), 17, t.nkmers, t.kmer, t.read, t.pos)
    return _cases["synth"]


def later_reads(c):
    """per tuple (k-mer, read): the reads > read that hold the k-mer = the count field of its B' entry"""
    key = c.tk.astype(np.int64) * (int(c.rs.nreads) + 1) + c.tr.astype(np.int64)
    key = np.unique(key)
    km = key // (int(c.rs.nreads) + 1)
    _, start, cnt = np.unique(km, return_index=True, return_counts=True)
    rank = np.arange(len(km)) - np.repeat(start, cnt)
    return np.repeat(cnt, cnt) - 1 - rank


def install(eng, c, pe, *, mode=0, boundary=False, **tune):
    set_mode(eng, mode)
    eng.set_tuning("product_entries", pe)
    for k, v in tune.items():
        eng.set_tuning(k, v)
    eng.set_reads(c.rs)
    if boundary:
        eng.set_B(c.k, c.nkmers, *c.B)
    else:
        eng.assemble_tuples(c.k, c.nkmers, c.tk, c.tr, c.tp)


def restore(eng, *names):
    set_mode(eng, 0)
    eng.set_tuning("product_entries")
    for k in names:
        eng.set_tuning(k)
    eng.set_column_range(0, 0xFFFFFFFF)
    eng.set_partition(0, 1)


def check_whole(eng, c):
    n, flops = eng.overlap(c.pars())
    pairs, ext, colptrC = eng.get_pairs()
    assert flops == int(c.flop.sum()) and n == len(c.exp)
    assert np.array_equal(colptrC, c.ecol.astype(np.uint64))
    check_pairs(pairs, ext, c.exp, c.rs.lengths, c.k)
    return pairs, ext, colptrC


def expect_form(eng, c, products):
    """memory().live_nnz counts the entries B' holds: the products in the per-product form, the entries with a later read otherwise"""
    lr = later_reads(c)
    assert int(lr.sum()) == int(c.flop.sum())
    assert eng.memory().live_nnz == (int(lr.sum()) if products else int((lr > 0).sum()))


@pytest.mark.parametrize("order", [0, 1024])
@pytest.mark.parametrize("inline", [32768, 65536])
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_golden_sets_per_product(eng, name, path, inline, order):
    c = golden_case(name)
    try:
        install(eng, c, 2, mode=path | inline | order)
        expect_form(eng, c, True)
        check_whole(eng, c)
    finally:
        restore(eng)


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_golden_sets_per_entry_and_same_B(eng, name):
    c = golden_case(name)
    try:
        install(eng, c, 1)
        expect_form(eng, c, False)
        B1 = eng.get_B()
        check_whole(eng, c)
        install(eng, c, 2)
        B2 = eng.get_B()
        for a, b, e in zip(B1, B2, c.B):
            assert np.array_equal(a, b) and np.array_equal(a, e)
    finally:
        restore(eng)


def test_layout_bytes_follow_the_form():
    c = golden_case("toy120")
    lr = later_reads(c)
    assert (lr >= 2).any()                     # an entry with two later reads: the per-product B' is longer than the per-entry one

    def measure(pe, debug=0, compact_b=0):
        e = Engine(0)                          # a fresh context: buffers only ever grow
        try:
            e.set_debug(debug)
            e.set_tuning("compact_b", compact_b)
            install_plain(e, c, pe)
            m = e.memory()
            n, flops = e.overlap(c.pars())
            pairs, ext, colptrC = e.get_pairs()
            return int(m.layout_B_bytes), int(m.live_nnz), (n, flops, pairs, ext, colptrC)
        finally:
            e.close()

    def install_plain(e, c, pe):
        e.set_tuning("product_entries", pe)
        e.set_reads(c.rs)
        e.assemble_tuples(c.k, c.nkmers, c.tk, c.tr, c.tp)

    b1, l1, r1 = measure(1)
    b2, l2, r2 = measure(2)
    b2n, l2n, r2n = measure(2, debug=2048)     # as if the buffer could not be had
    b1k, l1k, r1k = measure(1, compact_b=1)
    b2k, l2k, r2k = measure(2, compact_b=1)    # every entry kept: the per-entry form
    assert l1 == int((lr > 0).sum()) and l2 == int(lr.sum()) and l2 > l1
    assert b2 > b1
    assert (b2n, l2n) == (b1, l1)
    assert (b2k, l2k) == (b1k, l1k) and l1k == len(lr)
    for n, flops, pairs, ext, colptrC in (r1, r2, r2n, r1k, r2k):
        assert flops == int(c.flop.sum()) and n == len(c.exp) and np.array_equal(colptrC, c.ecol.astype(np.uint64))
        check_pairs(pairs, ext, c.exp, c.rs.lengths, c.k)


def test_synthetic_set_has_the_columns_it_is_for():
    f = synth_case().flop
    assert (f == 0).any() and (f == 1).any()
    # several X3 batches of the 128-thread class (two A' loads in flight per lane: 256 products per batch) with a ragged tail
    assert ((f > 256) & (f <= 384) & (f % 64 != 0)).any()
    # several batches of the 512-thread class (tiers up to 3,712 products with quarter-size key tables) ...
    assert ((f > 2048) & (f <= 2752)).any()
    # ... and of the 1,024-thread classes (tiers from 4,600 products up -- with half-size tables from 3,500 --, the CU's 81,920- and
    # 163,840-byte classes), a ragged last batch included
    big = (f > 3712) & (f <= 11008)
    assert big.any() and (f[big] % 2048 != 0).any()


@pytest.mark.parametrize("tune", [{}, {"lds_tiers": 64}, {"row_lists": 1}], ids=["default", "above-the-tiers", "row-lists"])
def test_synthetic_set(eng, tune):
    test_synthetic_set_has_the_columns_it_is_for()
    c = synth_case()
    try:
        install(eng, c, 2, **tune)
        expect_form(eng, c, True)
        if "row_lists" in tune:
            assert eng.memory().rowlist_bytes > 0          # built from the per-product B'
        check_whole(eng, c)
    finally:
        restore(eng, *tune)


def test_synthetic_set_global_path_and_inline(eng):
    c = synth_case()
    try:
        for mode in (65536, 1 | 65536, 32768):
            install(eng, c, 2, mode=mode)
            check_whole(eng, c)
    finally:
        restore(eng)


@pytest.mark.parametrize("name", ["toy120", "synth"])
def test_generic_readers_of_B(eng, name):
    """the symbolic phase (whole, column range, partition), the partitioned numeric pass and the drop-in boundary on a per-product B'"""
    c = synth_case() if name == "synth" else golden_case(name)
    nr = c.rs.nreads
    try:
        install(eng, c, 2)
        expect_form(eng, c, True)
        colptrC, n, flops = eng.count_pairs(c.pars())
        assert n == len(c.exp) and flops == int(c.flop.sum()) and np.array_equal(colptrC, c.ecol.astype(np.uint64))
        lo, hi = nr // 3, nr // 3 + max(1, nr // 2)
        eng.set_column_range(lo, hi - lo)
        colptrC, n, flops = eng.count_pairs(c.pars())
        own = np.zeros(nr, bool); own[lo:min(hi, nr)] = True
        assert np.array_equal(np.diff(colptrC.astype(np.int64)), np.where(own, c.ecnt, 0)) and flops == int(c.flop[own].sum())
        eng.set_column_range(0, 0xFFFFFFFF)
        eng.set_partition(1, 2)
        colptrC, n, flops = eng.count_pairs(c.pars())
        own = np.arange(nr) % 2 == 1
        assert np.array_equal(np.diff(colptrC.astype(np.int64)), np.where(own, c.ecnt, 0)) and n == int(c.ecnt[own].sum()) and flops == int(c.flop[own].sum())
        parts, exts = [], []
        for r in range(2):
            eng.set_partition(r, 2)
            n, flops = eng.overlap(c.pars())
            p, x, _ = eng.get_pairs()
            assert n == len(p) and (p["cid"] % 2 == r).all()
            parts.append(p); exts.append(x)
        merged, mext = np.concatenate(parts), np.concatenate(exts)
        order = np.argsort(merged["cid"], kind="stable")   # columns ascending, slot order kept inside a column
        check_pairs(merged[order], mext[order], c.exp, c.rs.lengths, c.k)
        eng.set_partition(0, 1)
        # the layout built FOR a partition (B' of the owned columns only)
        for r in range(2):
            eng.set_partition(r, 2)
            install(eng, c, 2)
            n, flops = eng.overlap(c.pars())
            p, x, _ = eng.get_pairs()
            assert np.array_equal(p, parts[r]) and np.array_equal(x, exts[r])
        eng.set_partition(0, 1)
        install(eng, c, 2, boundary=True)
        expect_form(eng, c, True)
        check_whole(eng, c)
    finally:
        restore(eng)


def test_switching_the_form_between_passes(eng):
    c = synth_case()
    try:
        got = []
        for pe in (1, 2, 1, 2):
            install(eng, c, pe)
            expect_form(eng, c, pe == 2)
            first = check_whole(eng, c)
            warm = check_whole(eng, c)                     # the remembered tier lengths belong to this layout
            for a, b in zip(first, warm):
                assert np.array_equal(a, b)
            got.append(first)
        for r in got[1:]:
            for a, b in zip(got[0], r):
                assert np.array_equal(a, b)
    finally:
        restore(eng)
