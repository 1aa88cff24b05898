"""The slot-order pass (order.hpp) on columns built for their PAIR COUNTS.  When two launches share the columns of a pass (order_split),
k_order_wave reads a column's records once and places them through LDS in windows of W ranks (W = 192 for tables of up to 512 slots,
384 for tables of up to 1,024); the single launch of a small pass gathers the records by rank.  What can go wrong depends on a column's
pair count d relative to 16, 64, W, 512 and 1,024.  Compared exactly as test_product_entries_gpu.py::check_whole compares: products,
pair count, colptrC, every record field, the diagnostics array, all against the oracle."""
import numpy as np
import pytest

import _oracle as O
from bella_amd import BellaPars, Engine, api
from bella_testkit import synth

pytestmark = pytest.mark.gpu

K = 17
SPACER = 20
# pair counts of the hub columns.  One chance pair can land in a hub column (a 17-mer of a spacer); the list and the seed are chosen so
# that the oracle's colptrC holds every count of REQUIRED (checked by has_the_columns before the device runs)
HUBS = [1, 15, 16, 17, 63, 64, 65, 191, 192, 193, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1500]
SEED = 8
REQUIRED = [1, 15, 16, 17, 63, 64, 65,          # one block of 64 records per lane and around it; the smallest table (16 slots)
            191, 192, 193, 383, 384, 385,       # window boundaries of W = 192 (tables of up to 512 slots, two launches)
            767, 768, 769,                      # ... and, with 383 .. 385, of W = 384 (tables of up to 1,024 slots)
            511, 512, 513,                      # the boundary between the two instances
            1023, 1024]                         # the largest table a wavefront orders
BIG = [1025, 1500]                              # k_order_block (unchanged) must still get its list


def hub_reads(hubs, seed):
    """reads 0 .. H-1: random hubs of 2 max(d) + 40 bases.  Read H + j: between 20-base random spacers the 17-mer hub[j : j + 17] of
    every hub with j < d, and for j % 3 == 0 a second 17-mer of the same hub from its upper half: pairs with two products, so records
    of the row kernels' two emitting phases interleave in slot order."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)
    dmax = max(hubs)
    hub = [bases[rng.integers(0, 4, 2 * dmax + 40)] for _ in hubs]
    seqs = [h.tobytes() for h in hub]
    for j in range(dmax):
        parts = []
        for h, d in zip(hub, hubs):
            if j >= d:
                continue
            parts += [bases[rng.integers(0, 4, SPACER)], h[j:j + K]]
            if j % 3 == 0:
                parts += [bases[rng.integers(0, 4, SPACER)], h[dmax + 20 + j:dmax + 20 + j + K]]
        parts.append(bases[rng.integers(0, 4, SPACER)])
        seqs.append(np.concatenate(parts).tobytes())
    return synth.readset_from_seqs(seqs)


class Case:
    """operands + the oracle's answer, computed once and shared (read-only)"""

    def __init__(self, hubs):
        self.rs = hub_reads(hubs, SEED)
        t = synth.count_and_tuples(self.rs, K, 2, 8)
        self.nkmers, self.tk, self.tr, self.tp = t.nkmers, t.kmer, t.read, t.pos
        B = O.build_B(self.rs.nreads, self.tk, self.tr, self.tp)
        flop, ecol, self.exp = O.spgemm(self.rs.seqs(), self.nkmers, *B, K)
        self.flop = np.asarray(flop).astype(np.int64)
        self.ecol = ecol.astype(np.uint64)
        self.ecnt = np.diff(ecol.astype(np.int64))
        for a in (self.flop, self.ecol, self.ecnt, self.exp):
            a.setflags(write=False)

    def pars(self):
        return BellaPars(skipAlignment=True, kmerSize=K)


_cases = {}


def case(which="whole"):
    if which not in _cases:
        _cases[which] = Case(HUBS if which == "whole" else HUBS[:-2])
    return _cases[which]


def has_the_columns(c, big=True):
    have = set(c.ecnt.tolist())
    missing = [d for d in REQUIRED + (BIG if big else []) if d not in have]
    assert not missing, missing
    assert big == bool((c.ecnt > 1024).any())
    # pairs with two products among the one-product pairs of a column
    assert (c.exp["count"] == 2).any() and (c.exp["count"] == 1).any()


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.set_debug(0)
    e.set_tuning("order_split")
    e.set_tuning("product_entries")
    e.set_partition(0, 1)
    e.close()


def install(eng, c, *, split=None, pe=None, debug=0):
    eng.set_debug(debug)
    eng.set_tuning("order_split", *([] if split is None else [split]))
    eng.set_tuning("product_entries", *([] if pe is None else [pe]))
    eng.set_reads(c.rs)
    eng.assemble_tuples(K, c.nkmers, c.tk, c.tr, c.tp)


def check_pairs(got, ext, exp, lengths):
    assert len(got) == len(exp)
    for f in ("rid", "cid", "count", "seedH", "seedV"):
        assert np.array_equal(got[f], exp[f]), f
    if ext is not None:
        for f in ("nbins", "support", "binov"):
            assert np.array_equal(ext[f], exp[f]), f
    assert np.array_equal(api.overlap_of_seed(got, lengths, K), exp["overlap"].astype(np.int64))


def check_whole(eng, c, ext=True):
    n, flops = eng.overlap(c.pars())
    pairs, x, colptrC = eng.get_pairs(ext=ext)
    assert flops == int(c.flop.sum()) and n == len(c.exp)
    assert np.array_equal(colptrC, c.ecol)
    check_pairs(pairs, x, c.exp, c.rs.lengths)
    return pairs


def test_hub_set_has_the_columns_it_is_for():
    has_the_columns(case())
    has_the_columns(case("small"), big=False)


@pytest.mark.parametrize("ext", [True, False], ids=["diagnostics", "records-only"])
@pytest.mark.parametrize("split", [None, 0], ids=["one-launch", "two-launches"])
def test_every_pair_count(eng, split, ext):
    c = case()
    has_the_columns(c)
    install(eng, c, split=split, debug=0 if ext else 2)     # bit 1: no diagnostics array, as in the timed path of bench.py
    check_whole(eng, c, ext=ext)


@pytest.mark.parametrize("split", [None, 0], ids=["one-launch", "two-launches"])
def test_partitions(eng, split):
    c = case()
    has_the_columns(c)
    install(eng, c, split=split)
    parts, exts = [], []
    try:
        for r in range(2):
            eng.set_partition(r, 2)
            n, _ = eng.overlap(c.pars())
            p, x, _ = eng.get_pairs()
            assert n == len(p) == int(c.ecnt[r::2].sum()) and (p["cid"] % 2 == r).all()
            parts.append(p); exts.append(x)
    finally:
        eng.set_partition(0, 1)
    merged, mext = np.concatenate(parts), np.concatenate(exts)
    order = np.argsort(merged["cid"], kind="stable")        # columns ascending, slot order kept inside a column
    check_pairs(merged[order], mext[order], c.exp, c.rs.lengths)


def test_per_entry_form(eng):
    c = case()
    has_the_columns(c)
    install(eng, c, split=0, pe=1)
    check_whole(eng, c)


@pytest.mark.parametrize("split", [None, 0], ids=["one-launch", "two-launches"])
def test_warm_pass_without_and_with_big_columns(eng, split):
    """a warm pass leaves k_order_block out when its predecessor listed no column for it: first a set without the two largest hubs
    (the second pass skips the kernel), then the whole set on the same context (both passes run it)"""
    small, c = case("small"), case()
    has_the_columns(small, big=False)
    has_the_columns(c)
    for cc in (small, c):
        install(eng, cc, split=split)
        first = check_whole(eng, cc)
        warm = check_whole(eng, cc)
        assert np.array_equal(first, warm)
