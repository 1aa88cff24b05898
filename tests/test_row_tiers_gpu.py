"""The row kernels (spgemm.hpp: k_spgemm_rows_lds, k_spgemm_rows_global, process_row) on columns built for the EDGES of every LDS tier
and key table (bella_testkit/tier_cases.py; tests/test_tier_cases_cpu.py shows that the sets have the columns they are for): key table
exactly full and one pair over, the dense list of multi-product pairs exactly full and one over, F == cap and cap +- 1, one list as long
as the tier, entries with several later reads, the four-range split around 256 products.  Compared exactly as
test_product_entries_gpu.py::check_whole compares -- products, pair count, colptrC, every record field, the diagnostics array -- against
the oracle, one oracle run per set."""
import numpy as np
import pytest

import _oracle as O
from bella_amd import BellaPars, Engine, api
from bella_testkit import tier_cases as T

pytestmark = pytest.mark.gpu

K = T.K
FORMS = {"per-entry": dict(product_entries=1, inline_entries=1),
         "inline": dict(product_entries=1, inline_entries=2),          # every hub entry has one later read: the inline branch of X3
         "per-product": dict(product_entries=2),
         "row-lists": dict(row_lists=1)}
TUNINGS = ("product_entries", "inline_entries", "row_lists", "lds_tiers")


class Case:
    """operands + the oracle's answer, computed once and shared (read-only)"""

    def __init__(self, t):
        self.t, self.rs = t, t.rs
        self.nkmers, self.tk, self.tr, self.tp = t.nkmers, t.tk, t.tr, t.tp
        B = O.build_B(self.rs.nreads, self.tk, self.tr, self.tp)
        flop, ecol, self.exp = O.spgemm(t.seqs, self.nkmers, *B, K)
        self.flop = np.asarray(flop).astype(np.int64)
        self.ecol = ecol.astype(np.uint64)
        reads = np.unique(self.tk, return_counts=True)[1]                     # (a k-mer appears once per read)
        self.live_entries = int((reads - 1).sum())                            # B' entries with a later read: all but a k-mer's last
        assert int((reads * (reads - 1) // 2).sum()) == int(self.flop.sum())
        for a in (self.flop, self.ecol, self.exp):
            a.setflags(write=False)

    def pars(self):
        return BellaPars(skipAlignment=True, kmerSize=K)


_cases = {}


def case(key, make):
    if key not in _cases:
        _cases[key] = Case(make())
    return _cases[key]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    restore(e)
    e.close()


def restore(eng):
    eng.set_debug(0)
    for name in TUNINGS:
        eng.set_tuning(name)


def install(eng, c, form, *, tiers=(), debug=0):
    restore(eng)
    eng.set_debug(debug)
    if tiers:
        eng.set_tuning("lds_tiers", *tiers)
    for name, v in FORMS[form].items():
        eng.set_tuning(name, v)
    eng.set_reads(c.rs)
    eng.assemble_tuples(K, c.nkmers, c.tk, c.tr, c.tp)


def expect_form(eng, c, form):
    """memory().live_nnz counts the entries B' holds: the products in the per-product form, the entries with a later read otherwise;
    the row lists exist in their form only"""
    m = eng.memory()
    assert m.live_nnz == (int(c.flop.sum()) if form == "per-product" else c.live_entries)
    assert (m.rowlist_bytes > 0) == (form == "row-lists")


def check_whole(eng, c):
    n, flops = eng.overlap(c.pars())
    pairs, ext, colptrC = eng.get_pairs()
    assert flops == int(c.flop.sum()) and n == len(c.exp)
    assert np.array_equal(colptrC, c.ecol)
    assert len(pairs) == len(c.exp)
    for f in ("rid", "cid", "count", "seedH", "seedV"):
        assert np.array_equal(pairs[f], c.exp[f]), f
    for f in ("nbins", "support", "binov"):
        assert np.array_equal(ext[f], c.exp[f]), f
    assert np.array_equal(api.overlap_of_seed(pairs, c.rs.lengths, K), c.exp["overlap"].astype(np.int64))
    return pairs, ext, colptrC


def cold_and_warm(eng, c, retries):
    """a pass, then a second one on the same operands: identical records, and the same count of columns handed to the global path"""
    first = check_whole(eng, c)
    assert eng.timings().retry_columns == retries
    warm = check_whole(eng, c)
    assert eng.timings().retry_columns == retries
    for a, b in zip(first, warm):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("regime,cap", [(r, C) for r in "QH" for C in T.CAPS[r]])
def test_single_tier(eng, regime, cap):
    """every hub of the tier in every form; retry_columns must be the number of columns DESIGNED with more pairs than the tier's key
    table holds (one, or none where the table is as large as the tier): that the count comes out proves that the regime and the dcap
    rule assumed here are the ones that ran.

    Single-tier runs (lds_tiers = C): the instantiation the tier's launch reaches, read from run_spgemm's dispatch (LDS bytes of (C, dcap)
    -> class -> block size -> NX); with debug bit 3 every class runs 512 threads.
        regime Q (dcap = C / 4)                               regime H (dcap = C up to 300, C / 2 up to 4,096, then C / 4)
          384                   <6,128>                         300                   <6,128>
          689, 1000, 1394       <6,256>                         526, 800, 1064        <6,256>
          2048, 2752, 3712      <8,512>                         1600, 2105, 2789      <8,512>
          4600, 5568, 8192      <8,1024>   bit 3: <16,512>      3500, 4096            <4,1024>
          11008                 <11,1024>  bit 3: <22,512>      6144                  <8,1024>   bit 3: <16,512>
    each as the per-entry kernel (plain and inline entries), the per-product kernel (PE) and the row-list kernel (RL).  The column of
    C + 1 products and the column whose pairs overflow the key table run in k_spgemm_rows_global."""
    c = case((regime, cap), lambda: T.edge_set(cap, regime))
    t = c.t
    retries = t.retries(cap, T.dcap_of(cap, regime))
    assert retries == sum(1 for h in t.hubs if h.name == "overflow")
    assert np.array_equal(c.flop[[h.col for h in t.hubs]], [h.F for h in t.hubs])
    try:
        for debug in (0, 8) if cap > 4096 else (0,):              # bit 3: 512 threads in every class
            for form in FORMS:
                install(eng, c, form, tiers=(cap,), debug=debug)
                expect_form(eng, c, form)
                cold_and_warm(eng, c, retries)
    finally:
        restore(eng)


@pytest.mark.parametrize("regime", ["Q", "H"])
def test_default_tables_all_tiers(eng, regime):
    """hubs of C - 1, C and C + 1 products for every tier of the regime's table, each with the pairs its OWN tier's table holds: pins
    k_tier_lists' f <= caps[t] and the walk over a class's tiers with the neighbouring tiers filled.  A class carves for its largest
    tier, so nothing overflows."""
    c = case(("table", regime), lambda: T.table_set(regime))
    try:
        for form in ("per-entry", "per-product"):
            install(eng, c, form)
            expect_form(eng, c, form)
            cold_and_warm(eng, c, 0)
    finally:
        restore(eng)


@pytest.mark.parametrize("regime", ["Q", "H"])
def test_one_class_more_than_four_tiers(eng, regime):
    """seven tiers in the smallest class, two of them empty: the launch reads the tiers' counts from the control block"""
    c = case(("small", regime), lambda: T.small_class_set(regime))
    try:
        for form in ("per-entry", "per-product"):
            install(eng, c, form, tiers=T.SMALL_CLASS_TIERS)
            expect_form(eng, c, form)
            cold_and_warm(eng, c, 0)
    finally:
        restore(eng)


@pytest.mark.parametrize("nsame,length,top", [(16, 4385, 65535), (17, 4112, 65536)])
def test_top_edge(eng, nsame, length, top):
    """identical reads: the first has 65,535 products -- the last column of the tier above the LDS tiers, every packed 16-bit count at
    its maximum -- or 65,536, the first column of the wide path.  They stand on ids the sample does not see (tier_cases.top_edge_set):
    quarter tables, every default tier open, no row lists on their own, so product_entries selects the form that runs.  13 columns lie
    above the LDS tiers (fewer than 16: k_spgemm_rows_global<false>; with debug bit 5 the sort-based path)."""
    c = case(("top", nsame), lambda: T.top_edge_set(nsame, length))
    cols = c.t.same_cols
    assert int(c.flop[cols[0]]) == top and int(c.flop.max()) == top
    assert [int(f) for f in c.flop[cols]] == [(length - K + 1) * (nsame - 1 - x) for x in range(nsame)]
    assert int(((c.flop > 11008) & (c.flop <= 65535)).sum()) == 13
    try:
        for debug in (0, 32):
            for form in ("per-entry", "per-product"):
                install(eng, c, form, debug=debug)
                expect_form(eng, c, form)
                cold_and_warm(eng, c, 0)
    finally:
        restore(eng)
