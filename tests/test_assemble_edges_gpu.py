"""Operand assembly (assemble.hpp, slotorder.hpp; bella_hip.hip: assemble_rows_device, build_layout) on sets built for the EDGES of its
table classes, insertion rounds, probe chains, LDS windows, chunks and rounds (bella_testkit/assemble_cases.py;
tests/test_assemble_cases_cpu.py shows that the sets hold the geometry they are for).  Rows: get_B() against the oracle's B, array for
array.  Layouts: compared exactly as test_row_tiers_gpu.check_whole compares -- products, pair count, colptrC, every record field, the
diagnostics array, overlap_of_seed -- in every form of B' / A', one oracle run per set; and the seed flags of every record (same strand,
reverse complement; both for a palindrome) against the bases, which is where the palindrome bit of a B' entry ends up.
Engine.assemble_stats() must report the table classes, the entry form, the list order and the place pass the mirror states, so a set
that lands on another path fails.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from conftest import load_golden
from bella_amd import BellaHipError, BellaPars, Engine, api
from bella_testkit import assemble_cases as A
from bella_testkit import assemble_mirror as M

pytestmark = pytest.mark.gpu

# form -> tuning values, debug word (bit 10: the lists of A' in first-appearance order)
FORMS = {
    "plain": (dict(inline_entries=1, product_entries=1), 0),
    "inline": (dict(inline_entries=2, product_entries=1), 0),
    "per-product": (dict(inline_entries=1, product_entries=2), 0),
    "per-product-inline": (dict(inline_entries=2, product_entries=2), 0),
    "dead-kept": (dict(inline_entries=1, product_entries=1, compact_b=1), 0),
    "dead-kept-inline": (dict(inline_entries=2, product_entries=1, compact_b=1), 0),
    "first-appearance": (dict(inline_entries=1, product_entries=1), 1024),
    "first-appearance-inline": (dict(inline_entries=2, product_entries=2), 1024),
    "row-lists": (dict(inline_entries=1, row_lists=1), 0),
    "row-lists-inline": (dict(inline_entries=2, row_lists=1), 0),
    "row-lists-dead-kept": (dict(inline_entries=2, row_lists=1, compact_b=1), 0),
}
TUNINGS = ("product_entries", "inline_entries", "row_lists", "compact_b", "lds_tiers")
BAD_ARG, READ_TOO_LONG, TUPLE_ORDER = -3, -5, -6


class Answer:
    """a case + the oracle's answer, computed once and shared (read-only)"""

    def __init__(self, c, spgemm=True):
        self.c, self.rs, self.k = c, c.rs, c.k
        self.B = O.build_B(c.rs.nreads, c.tk, c.tr, c.tp)
        self.classes = M.class_counts(c.rows())
        if spgemm:
            flop, ecol, self.exp = O.spgemm(c.seqs, c.nkmers, *self.B, c.k)
            self.flop = np.asarray(flop).astype(np.int64)
            self.ecol = ecol.astype(np.uint64)
            self.ecnt = np.diff(ecol.astype(np.int64))
            for a in (self.flop, self.ecol, self.exp):
                a.setflags(write=False)
        for a in self.B:
            a.setflags(write=False)
        # the 2-bit codes of every k-mer of every read, both strands, side by side: what the seed flags of a record are checked against
        codes = [M.kmer_codes(s, c.k) for s in c.seqs]
        self.koff = np.concatenate([[0], np.cumsum([len(f) for f, _ in codes])])
        self.kfw = np.concatenate([f for f, _ in codes])
        self.krc = np.concatenate([r for _, r in codes])

    def seed_flags(self, pairs):
        """bit 0: the seed k-mers of the two reads are equal base for base; bit 1: one is the reverse complement of the other (both for
        a palindrome) -- from the sequences"""
        h = self.koff[pairs["rid"]] + pairs["seedH"]
        v = self.koff[pairs["cid"]] + pairs["seedV"]
        return (self.kfw[h] == self.kfw[v]).astype(np.uint16) | ((self.krc[h] == self.kfw[v]).astype(np.uint16) << 1)

    def pars(self):
        return BellaPars(skipAlignment=True, kmerSize=self.k)


_answers = {}


def answer(name, spgemm=True):
    if name not in _answers:
        _answers[name] = Answer(A.case(name), spgemm)
    return _answers[name]


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
    eng.set_partition(0, 1)
    eng.set_column_range(0, 0xFFFFFFFF)


def install(eng, a, form, part=(0, 1)):
    restore(eng)
    tun, debug = FORMS[form]
    eng.set_debug(debug)
    for name, v in tun.items():
        eng.set_tuning(name, v)
    eng.set_partition(*part)
    eng.set_reads(a.rs)
    eng.assemble_tuples(a.k, a.c.nkmers, a.c.tk, a.c.tr, a.c.tp)


def expect_path(eng, a, form, part=(0, 1)):
    """assemble_stats() and memory() against the mirror: the table classes of the rows, the form of B', the order of A', the place pass"""
    L = a.c.layout(a.B, *part)
    tun, debug = FORMS[form]
    st, m = eng.assemble_stats(), eng.memory()
    products = tun.get("product_entries") == 2 and not tun.get("compact_b") and L.products() > 0
    assert st["classes"] == a.classes
    assert st["inline"] == (tun["inline_entries"] == 2)
    assert st["products"] == products
    assert st["first_appearance"] == bool(debug & 1024)
    assert st["place_sorted"] == L.place_sorts
    assert m.live_nnz == (L.products() if products else L.nown if tun.get("compact_b") else L.live_entries())
    assert (m.rowlist_bytes > 0) == ("row_lists" in tun)


def check_whole(eng, a):
    n, flops = eng.overlap(a.pars())
    pairs, ext, colptrC = eng.get_pairs()
    assert flops == int(a.flop.sum()) and n == len(a.exp)
    assert np.array_equal(colptrC, a.ecol)
    check_records(pairs, ext, a.exp, a)


def check_records(pairs, ext, exp, a):
    assert len(pairs) == len(exp)
    for f in ("rid", "cid", "count", "seedH", "seedV"):
        assert np.array_equal(pairs[f], exp[f]), f
    for f in ("nbins", "support", "binov"):
        assert np.array_equal(ext[f], exp[f]), f
    assert np.array_equal(api.overlap_of_seed(pairs, a.rs.lengths, a.k), exp["overlap"].astype(np.int64))
    assert np.array_equal(pairs["flags"], a.seed_flags(pairs))


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.names(*A.ROW_FAMILIES) + ["row_limits_max"])
def test_rows(eng, name):
    """get_B() equals the oracle's B array for array; the five class counts are the mirror's"""
    a = answer(name, spgemm=False)
    try:
        install(eng, a, "plain")
        assert eng.assemble_stats()["classes"] == a.classes
        for got, exp in zip(eng.get_B(), a.B):
            assert np.array_equal(got, exp)
    finally:
        restore(eng)


def test_rows_twice_on_one_engine(eng):
    """the global class's workspace and the class lists are re-used: a second assembly of another set, then the first again"""
    try:
        for name in ("row_probes", "row_duplicates", "row_probes"):
            a = answer(name, spgemm=False)
            install(eng, a, "plain")
            for got, exp in zip(eng.get_B(), a.B):
                assert np.array_equal(got, exp)
    finally:
        restore(eng)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = A.names(*A.LAYOUT_FAMILIES)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_layout(eng, name, form):
    a = answer(name)
    try:
        install(eng, a, form)
        expect_path(eng, a, form)
        check_whole(eng, a)
    finally:
        restore(eng)


@pytest.mark.parametrize("form", ["plain", "inline", "per-product", "row-lists"])
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_layout_partitioned(eng, name, form):
    """set_partition(f, 3) BEFORE the assembly, so that the layout itself is the partition's (k_layout_emit's workgroups of 1,024, the
    owned entries compacted, the place pass over a third of the entries); the union of the three equals the whole"""
    a = answer(name)
    parts, exts = [], []
    try:
        for f in range(3):
            install(eng, a, form, part=(f, 3))
            expect_path(eng, a, form, part=(f, 3))
            own = np.arange(a.rs.nreads) % 3 == f
            n, flops = eng.overlap(a.pars())
            p, x, colptrC = eng.get_pairs()
            assert n == len(p) == int(a.ecnt[own].sum()) and flops == int(a.flop[own].sum())
            assert np.array_equal(np.diff(colptrC.astype(np.int64)), np.where(own, a.ecnt, 0))
            assert (p["cid"] % 3 == f).all()
            parts.append(p)
            exts.append(x)
    finally:
        restore(eng)
    merged, mext = np.concatenate(parts), np.concatenate(exts)
    order = np.argsort(merged["cid"], kind="stable")               # columns ascending, slot order kept inside a column
    check_records(merged[order], mext[order], a.exp, a)


# ---- panels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [(0, 500, 1200), (0, 0, 700, 1200), (0, 333, 334, 1200)], ids=["two", "empty-first", "three"])
def test_runs_in_panels(eng, bounds):
    """`runs` assembled in row-block panels with uneven bounds (an empty panel among them), concatenated on the device, handed back through
    set_B_device: the same B and the same records"""
    import torch
    a = answer("runs")
    c = a.c
    assert bounds[-1] == c.rs.nreads
    try:
        restore(eng)
        eng.set_reads(a.rs)
        parts = []
        for lo, hi in zip(bounds, bounds[1:]):
            sel = (c.tr >= lo) & (c.tr < hi)
            eng.assemble_panel(a.k, c.nkmers, lo, hi - lo, c.tk[sel], c.tr[sel], c.tp[sel])
            parts.append([t.clone() for t in eng.panel_tensors(0)])
        cnt, ids, val = (torch.cat([p[x] for p in parts]) for x in range(3))
        colptr = torch.zeros(cnt.numel() + 1, dtype=torch.int32, device=cnt.device)
        colptr[1:] = torch.cumsum(cnt, 0).to(torch.int32)
        eng.set_B_device(a.k, c.nkmers, colptr, ids, val)
        for got, exp in zip(eng.get_B(), a.B):
            assert np.array_equal(got, exp)
        check_whole(eng, a)
    finally:
        restore(eng)


def test_panel_starting_at_a_read_without_tuples(eng):
    """row_classes: panels whose first read, and whose last read, have no tuples"""
    import torch
    a = answer("row_classes", spgemm=False)
    c = a.c
    g = c.rows()
    empty = [r for r in range(1, c.rs.nreads - 1) if r not in g]
    assert empty
    bounds = (0, empty[0], empty[-1] + 1, c.rs.nreads)             # panel 0 starts at the empty read 0, panel 1 at an empty read
    try:
        restore(eng)
        eng.set_reads(a.rs)
        parts = []
        for lo, hi in zip(bounds, bounds[1:]):
            sel = (c.tr >= lo) & (c.tr < hi)
            eng.assemble_panel(a.k, c.nkmers, lo, hi - lo, c.tk[sel], c.tr[sel], c.tp[sel])
            parts.append([t.clone() for t in eng.panel_tensors(0)])
        cnt, ids, val = (torch.cat([p[x] for p in parts]) for x in range(3))
        colptr = torch.zeros(cnt.numel() + 1, dtype=torch.int32, device=cnt.device)
        colptr[1:] = torch.cumsum(cnt, 0).to(torch.int32)
        eng.set_B_device(a.k, c.nkmers, colptr, ids, val)
        for got, exp in zip(eng.get_B(), a.B):
            assert np.array_equal(got, exp)
    finally:
        restore(eng)


# ---- limits -------------------------------------------------------------------------------------------------------------------------
def golden_still_assembles(eng):
    g = load_golden("toy120")
    eng.set_reads(g.rs)
    eng.assemble_tuples(g.k, g.nkmers, g.tk, g.tr, g.tp)
    for got, exp in zip(eng.get_B(), O.build_B(g.rs.nreads, g.tk, g.tr, g.tp)):
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("name,code", [("row_limits_over", READ_TOO_LONG), ("row_limits_order", TUPLE_ORDER)])
def test_row_errors(eng, name, code):
    """65,536 tuples in one read (status bit 16) and read ids that decrease (status bit 8): the error, then a correct assembly"""
    c = A.case(name)
    try:
        restore(eng)
        eng.set_reads(c.rs)
        with pytest.raises(BellaHipError) as e:
            eng.assemble_tuples(c.k, c.nkmers, c.tk, c.tr, c.tp)
        assert e.value.code == code
        golden_still_assembles(eng)
    finally:
        restore(eng)


@pytest.mark.parametrize("form", ["plain", "first-appearance"])
def test_degree_16384_is_refused(eng, form):
    """a k-mer in 16,384 reads (status bit 64), in both orders of A'; then a correct assembly"""
    c = A.case("degree_16384")
    tun, debug = FORMS[form]
    try:
        restore(eng)
        eng.set_debug(debug)
        eng.set_reads(c.rs)
        with pytest.raises(BellaHipError) as e:
            eng.assemble_tuples(c.k, c.nkmers, c.tk, c.tr, c.tp)
        assert e.value.code == BAD_ARG and "16383" in str(e.value)
        eng.set_debug(0)
        golden_still_assembles(eng)
    finally:
        restore(eng)


def oracle_columns(a, lo, hi):
    """the oracle's records of the columns lo .. hi - 1 alone (the symbolic and the numeric phase of a column range)"""
    c = a.c
    nr = c.rs.nreads
    Bc, Br, Bv = a.B
    Ac, Ar, Av = O.transpose(nr, c.nkmers, Bc, Br, Bv)
    arr = (C.c_char_p * nr)(*[bytes(s) for s in c.seqs])
    O._PAR.update(nreads=nr, Bc=Bc, Br=O._pad(Br, np.uint32), Bv=O._pad(Bv, np.uint16), Ac=Ac, Ar=O._pad(Ar, np.uint32), Av=O._pad(Av, np.uint16),
                  k=c.k, bin=500, arr=arr, lens=np.asarray([len(s) for s in c.seqs], np.uint32))
    try:
        _, _, flop, nnzc = O._sym_job((lo, hi))
        full = np.zeros(nr, np.uint32)
        full[lo:hi] = nnzc
        O._PAR["nnzc"] = full
        return flop.astype(np.int64), nnzc.astype(np.int64), O._num_job(np.arange(lo, hi))
    finally:
        O._PAR.clear()


@pytest.mark.parametrize("form", ["plain", "inline", "per-product", "first-appearance"])
def test_degree_16383(eng, form):
    """one k-mer in 16,383 reads: the largest count a B' entry holds.  The products of ALL columns against the closed form of the
    design; the records of the first and the last 8 columns against the oracle (134 M products are too many for the oracle)."""
    a = answer("degree_16383", spgemm=False)
    c = a.c
    nr = c.rs.nreads
    try:
        install(eng, a, form)
        L = c.layout(a.B)
        assert int(L.degree.max()) == M.MAX_DEGREE and L.products() == c.design["flops"]
        assert eng.assemble_stats()["classes"] == a.classes
        assert eng.count_flops(a.pars()) == c.design["flops"]
        for lo, hi in ((0, 8), (nr - 8, nr)):
            flop, nnzc, exp = oracle_columns(a, lo, hi)
            eng.set_column_range(lo, hi - lo)
            n, flops = eng.overlap(a.pars())
            pairs, ext, colptrC = eng.get_pairs()
            assert n == int(nnzc.sum()) and flops == int(flop.sum())
            own = np.zeros(nr, np.int64)
            own[lo:hi] = nnzc
            assert np.array_equal(np.diff(colptrC.astype(np.int64)), own)
            check_records(pairs, ext, exp, a)
    finally:
        restore(eng)
