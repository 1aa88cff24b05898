"""The path of the columns above the LDS tiers (bella_amd/csrc/wide.hpp) at the edges of its fold classes and tables, on the sets of
bella_testkit/wide_cases.py (tests/test_wide_cases_cpu.py shows that the sets have the pairs they are for): list lengths on both
sides of every threshold of k_wide_fold_wg (16 | 17, 96 | 97, 128 | 129, 1,024 | 1,025, 2,048 | 2,049, 4,096 | 4,097, 32,767 | 32,768) as
plain chains -- dense and sparse -- and on two, 16 and 17 diagonals; 65,535-base reads with products where the position grid's bucket
range wraps; columns on both sides of a chunk and of a round of the LDS grouping and of its table's 1,536 partners; more pairs than
the short-list instance has workgroups.

Every run has lds_tiers = 64 and debug bit 5: every column of 65 or more products takes the path.  Compared exactly as
test_row_tiers_gpu.check_whole compares -- products, pair count, colptrC, every field of EVERY record, nbins / support / binov, the
overlap of the seed -- against the oracle, one oracle run per set; a cold and a warm pass, identical.  bella_timings.wide_batches says
which grouping ran: the result is the same either way, so only the field can tell a batch that silently took the sort-based path."""
import numpy as np
import pytest

import test_row_tiers_gpu as R
from bella_testkit import wide_cases as W

pytestmark = pytest.mark.gpu

WIDE, SORT, KEY64 = 32, 4096, 64              # debug bits: columns above the tiers to wide.hpp; no LDS grouping; 64-bit sort keys
# route: debug bits, tunings, what wide_batches (grouped, sorted) must satisfy
ROUTES = {"lists-per-batch": (WIDE, {}, lambda g, s: g >= 1 and s == 0),
          "context-row-lists": (WIDE, dict(row_lists=1), lambda g, s: g >= 1 and s == 0),
          "sort-32": (WIDE | SORT, {}, lambda g, s: g == 0 and s >= 1),
          "sort-64": (WIDE | SORT | KEY64, {}, lambda g, s: g == 0 and s >= 1),
          "batches": (WIDE, dict(wide_budget=None), lambda g, s: g + s >= 3)}
FORMS = ("per-entry", "inline", "per-product")                              # the B' forms k_layout_rowlists / k_wide_expand read
# several batches: 40,000 products per batch; the long reads' columns hold 21,084 together and get 6,000 (their largest has 2,751)
BUDGET = {"fold": 40000, "long": 6000}
SETS = {"fold": W.fold_set, "long": W.long_read_set, "group": lambda: W.group_set(False), "group-over": lambda: W.group_set(True),
        "many": W.many_pairs_set}


@pytest.fixture(scope="module")
def eng():
    e = R.Engine(0)
    yield e
    restore(e)
    e.close()


def restore(eng):
    R.restore(eng)
    eng.set_tuning("wide_budget")


def install(eng, c, debug, tunings, form=None):
    restore(eng)
    eng.set_debug(debug)
    eng.set_tuning("lds_tiers", 64)
    for name, v in dict(R.FORMS[form] if form else {}, **tunings).items():
        eng.set_tuning(name, v)
    eng.set_reads(c.rs)
    eng.assemble_tuples(R.K, c.nkmers, c.tk, c.tr, c.tp)


def batches(eng):
    w = eng.timings().wide_batches
    return w & 0xFFFF, w >> 16


def cold_and_warm(eng, c, ok):
    """a pass, then a second one on the same operands: every record against the oracle, the two passes identical, no column handed
    to the global-workspace path, and wide_batches as the route demands -- after either pass (the field is of the LAST pass)"""
    first = R.check_whole(eng, c)
    g1 = batches(eng)
    assert eng.timings().retry_columns == 0
    warm = R.check_whole(eng, c)
    g2 = batches(eng)
    for a, b in zip(first, warm):
        assert np.array_equal(a, b)
    assert ok(*g1) and g1 == g2, (g1, g2)
    return g1


def run(eng, key, route, form=None, budget=None, ok=None):
    c = R.case(("wide", key), SETS[key])
    debug, tunings, route_ok = ROUTES[route]
    tunings = {n: (budget if v is None else v) for n, v in tunings.items()}
    try:
        install(eng, c, debug, tunings, form)
        if form:
            R.expect_form(eng, c, form)
        assert (eng.memory().rowlist_bytes > 0) == (route == "context-row-lists")
        return c, cold_and_warm(eng, c, ok or route_ok)
    finally:
        restore(eng)


FOLD_RUNS = [(r, f) for r in ("lists-per-batch", "sort-32") for f in FORMS] + [(r, None) for r in ("context-row-lists", "sort-64", "batches")]


@pytest.mark.parametrize("route,form", FOLD_RUNS)
def test_fold_classes(eng, route, form):
    """fold_set: a pair on every route of k_wide_fold_wg (wide_cases.fold_route), plain and not, 16 roots kept and 17 handed over in
    every instance and unstaged; the one-lane fold for lists of up to 16 and of 32,768 products"""
    c, _ = run(eng, "fold", route, form, BUDGET["fold"])
    t = c.t
    assert int(c.flop.max()) == W.FOLD_SERIAL and int((c.flop > 64).sum()) == len(t.hubs) + 1
    nb = c.exp["nbins"]
    assert int((nb == 17).sum()) == len(W.FOLD_MANY) == int((nb == 16).sum())


@pytest.mark.parametrize("route,form", FOLD_RUNS)
def test_long_reads(eng, route, form):
    """long_read_set: 65,535-base reads, products at position 0, at len - k and around every multiple of the grid's period, in all
    three instances, on one diagonal and on two, both strands"""
    c, _ = run(eng, "long", route, form, BUDGET["long"])
    assert int(c.rs.lengths.max()) == W.MAXLEN and int((c.exp["nbins"] == 2).sum()) == 2 * len(W.LONG_M)


@pytest.mark.parametrize("route", ["lists-per-batch", "context-row-lists"])
def test_grouping_at_chunk_round_and_table_edges(eng, route):
    """group_set(False): 1,536 partners fit the table -- no batch may leave the LDS grouping"""
    c, _ = run(eng, "group", route)
    assert int(np.diff(c.ecol.astype(np.int64)).max()) == W.GROUP_PAIRS


@pytest.mark.parametrize("route", ["lists-per-batch", "context-row-lists"])
def test_one_partner_more_than_the_table_holds(eng, route):
    """group_set(True) in one batch: the column of 1,537 partners raises the flag and the WHOLE batch takes the sort-based path"""
    c, _ = run(eng, "group-over", route, ok=lambda g, s: g == 0 and s >= 1)
    assert int(np.diff(c.ecol.astype(np.int64)).max()) == W.GROUP_PAIRS + 1


def test_one_partner_more_in_a_batch_of_its_own(eng):
    """... and with a budget that leaves that column alone in its batch, only that batch does"""
    run(eng, "group-over", "batches", budget=W.OVER_F, ok=lambda g, s: g >= 1 and s >= 1)


def test_more_pairs_than_workgroups(eng):
    """many_pairs_set: 8 x 16,384 + 8 pairs of 17 products (and the ballast's ten): a workgroup of the short-list instance folds more
    than eight pairs"""
    c, _ = run(eng, "many", "lists-per-batch")
    assert int((c.flop == W.MANY_M * W.MANY_PER_HUB).sum()) * W.MANY_PER_HUB == 8 * W.FOLD_GRID + 8
