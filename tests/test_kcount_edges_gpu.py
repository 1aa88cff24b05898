"""K-mer counting on the sets of bella_testkit/kcount_cases.py (run with `-m gpu` on an MI355X): (nkmers, ntuples, ndistinct), the
dictionary and the three tuple arrays against the C oracle, bit for bit, and what the host decided -- path, position bits, left-out
word bits, passes with their bins, words and tiles, slots of the look-up table -- against bella_testkit/kcount_mirror.py, so that a
change of the host's rules that leaves the cases' labels stale fails here instead of passing on another path.
tests/test_kcount_cases_cpu.py shows what each set holds.  One case of each family goes on through assemble_counted() and an overlap
without alignment, against the oracle's pairs.  Every comparison is an equality."""
import numpy as np
import pytest

import _oracle as O
from bella_amd import BellaPars, Engine
from bella_testkit import kcount_cases as KC
from bella_testkit import kcount_mirror as M
from conftest import set_mode
from test_kcount_cases_cpu import oracle_count

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def count_case(eng, c):
    """the case's count with its tuning value and debug bits, both restored; returns (nk, nt, nd), count_stats()"""
    eng.set_reads(c.rs)
    try:
        set_mode(eng, c.debug)
        eng.set_tuning("kcount_budget", c.budget)
        got = eng.count_kmers(c.k, c.lower, c.upper, c.mode == 1, c.window if c.mode == 2 else 0)
        return got, eng.count_stats()
    finally:
        set_mode(eng, 0)
        eng.set_tuning("kcount_budget")


def same_as_oracle_and_mirror(eng, c):
    what = (c.family, c.name)
    (nk, nt, nd), st = count_case(eng, c)
    codes, counts, tk, tr, tp, ndist = oracle_count(c)
    assert (nk, nt, nd) == (len(codes), len(tk), ndist), what
    dc, dn = eng.get_dictionary()
    assert np.array_equal(dc, codes), what
    assert np.array_equal(dn, counts), what
    gk, gr, gp = eng.get_tuples()
    assert np.array_equal(gk, tk) and np.array_equal(gr, tr) and np.array_equal(gp, tp), what
    d = c.describe()
    assert (st["fast"], st["pb"], st["gb"]) == (d["fast"], d["pb"], d["gb"]), what
    assert st["mode"] == c.mode and st["positions"] == d["counted"].npositions and st["slots"] == d["slots"], what
    assert [p[:3] for p in st["passes"]] == [tuple(p) for p in d["passes"]], what
    assert [p[3] for p in st["passes"]] == d["tiles"], what
    return nt


def run_cases(eng, cases):
    assert cases
    tuples = sum(same_as_oracle_and_mirror(eng, c) for c in cases)
    print("%d cases, %d reads, %d tuples compared" % (len(cases), sum(c.rs.nreads for c in cases), tuples))


@pytest.mark.parametrize("k", [17, 16, 13])
def test_tile_edges(eng, k):
    run_cases(eng, [c for c in KC.family("tile_edges") if c.k == k])


@pytest.mark.parametrize("k", [17, 13, 5])
def test_masks(eng, k):
    run_cases(eng, [c for c in KC.family("masks") if c.k == k])


@pytest.mark.parametrize("family", ["dense", "fast_limit", "lookup", "minimizer_ring", "small_k", "emit_chunks", "multi_pass"])
def test_family(eng, family):
    run_cases(eng, KC.family(family))


@pytest.mark.parametrize("part", ["base", "next-head", "count"])
def test_long_runs(eng, part):
    run_cases(eng, [c for c in KC.family("long_runs") if c.name.startswith(part)])


@pytest.mark.parametrize("mode", [1, 2])
def test_saturation(eng, mode):
    run_cases(eng, [c for c in KC.family("saturation") if c.mode == mode])


def test_stats_follow_the_last_count(eng):
    """two counts on one engine: the stats are those of the last one"""
    a, b = KC.family("dense")[0], KC.family("lookup")[0]
    _, sa = count_case(eng, a)
    _, sb = count_case(eng, b)
    assert sa["fast"] and not sb["fast"] and sb["slots"] == M.table_slots(511) == 1024 and sa["slots"] == 0
    assert sa["passes"] == [(0, 256, 2048, 1)] and sb["passes"] == [(0, 256, b.rs.nreads, 0)]
    assert sa["budget"] == sb["budget"] == 1 << 30


PIPELINE = {"tile_edges": "k17-head-e2047", "masks": "k17-low-pre7-a20-m1", "dense": "1024-pairs", "long_runs": "count-65536-u65535",
            "saturation": "m2-65536-u65534", "fast_limit": "k25-16384", "lookup": "debug14-k17-dict-512", "minimizer_ring": "k17-w3-r65",
            "small_k": "all-k6", "emit_chunks": "all-budget", "multi_pass": "masks"}


@pytest.mark.parametrize("family", list(PIPELINE))
def test_counted_case_through_assembly_and_overlap(eng, family):
    """count -> assemble_counted -> overlap on the device against the oracle's SpGEMM on the oracle's tuples: the ids must be the oracle's,
    a permutation of them would pair other reads at other seeds"""
    c = next(x for x in KC.family(family) if x.name == PIPELINE[family])
    (nk, nt, _), _ = count_case(eng, c)
    codes, counts, tk, tr, tp, _ = oracle_count(c)
    assert nk == len(codes) > 0 and nt == len(tk) > 0
    eng.assemble_counted()
    n, flops = eng.overlap(BellaPars(kmerSize=c.k, skipAlignment=True))
    pairs, _, _ = eng.get_pairs(ext=False)
    Bc, Br, Bv = O.build_B(c.rs.nreads, tk, tr, tp)
    flop, _, exp = O.spgemm(c.rs.seqs(), nk, Bc, Br, Bv, c.k)
    assert n == len(exp) and flops == int(flop.astype(np.int64).sum())
    for f in ("rid", "cid", "count", "seedH", "seedV"):
        assert np.array_equal(pairs[f], exp[f]), (family, c.name, f)
    print("%s/%s: %d reliable k-mers, %d tuples, %d pairs" % (family, c.name, nk, nt, n))
