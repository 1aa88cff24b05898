"""The case tables of tests/test_assemble_edges_gpu.py (bella_testkit/assemble_cases.py) without a GPU: the mirror's statement of a
read's row -- the slot order it simulates for the probe and round counts -- equals the oracle's B; every set keeps the rule that two
tuples carry the same id if and only if the bases at their positions are the same canonical k-mer; and a census: the families
together hold every table class, round, probe, window, chunk and round geometry the GPU file is there to run.  The census reads the
sets through the mirror; it does not trust the builders."""
import os

import numpy as np
import pytest

import _oracle as O
from bella_testkit import assemble_cases as A
from bella_testkit import assemble_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_CASES = A.names(*A.ROW_FAMILIES) + ["row_limits_max"]
LAYOUT_CASES = A.names(*A.LAYOUT_FAMILIES)
ALL_CASES = A.names(*A.FAMILIES)

_B = {}


def oracle_B(name):
    if name not in _B:
        c = A.case(name)
        _B[name] = O.build_B(c.rs.nreads, c.tk, c.tr, c.tp)
    return _B[name]


@pytest.mark.parametrize("name", ROW_CASES)
def test_mirror_rows_equal_oracle(name):
    c = A.case(name)
    Bc, Br, Bv = oracle_B(name)
    g = c.rows()
    starts = np.searchsorted(c.tr, np.arange(c.rs.nreads + 1))
    assert np.array_equal(np.diff(Bc.astype(np.int64)), [g[r].d if r in g else 0 for r in range(c.rs.nreads)])
    for r, x in g.items():
        km, pos = x.row(c.tk[starts[r]:starts[r + 1]], c.tp[starts[r]:starts[r + 1]])
        assert np.array_equal(km, Br[Bc[r]:Bc[r + 1]]) and np.array_equal(pos, Bv[Bc[r]:Bc[r + 1]]), r
        assert sum(x.round_items) == x.d and x.bounds[-1] == x.n and all(a < b for a, b in zip(x.bounds, x.bounds[1:]))


@pytest.mark.parametrize("name", ALL_CASES)
def test_ids_follow_the_sequences(name):
    """same id <=> same canonical k-mer at the positions, from the sequences and the tuples alone; every k-mer lies inside its read"""
    c = A.case(name)
    canon = np.zeros(len(c.tk), np.uint64)
    starts = np.searchsorted(np.sort(c.tr), np.arange(c.rs.nreads + 1))
    order = np.argsort(c.tr, kind="stable")                       # (row_limits_order hands its tuples over in decreasing read order)
    for r in range(c.rs.nreads):
        t = order[starts[r]:starts[r + 1]]
        if len(t):
            assert int(c.tp[t].max()) + c.k <= len(c.seqs[r])
            fw, rc = M.kmer_codes(c.seqs[r], c.k)
            canon[t] = np.minimum(fw, rc)[c.tp[t]]
    ids, kmers = np.unique(c.tk), np.unique(canon)
    both = np.unique(np.stack([c.tk.astype(np.uint64), canon]), axis=1).shape[1]
    assert len(ids) == len(kmers) == both
    assert int(c.tk.max()) < c.nkmers


def test_a_chance_collision_raises():
    b = A.Builder(A.K, 0)
    s, ky = b.stretch(3)
    b.read([b.seg(s, ky)])
    b.read([(s, np.arange(3), b.keys(3))])                        # the same bases under three new keys
    with pytest.raises(ValueError):
        b.finish("x", "x")
    b = A.Builder(A.K, 0)
    s, ky = b.stretch(3)
    b.read([b.seg(s, ky), (b.bases(A.K), np.zeros(1, np.int64), ky[:1])])   # one key on two different k-mers
    with pytest.raises(ValueError):
        b.finish("x", "x")


ROW_KEYS = {
    "row_classes": ["n=%d" % n for n in A.ROW_SIZES] + ["class-%d" % q for q in range(5)] +
                   ["load-1.0-ht=%d" % h for h in (16, 128, 1024, 2048, 4096, 8192)] +
                   ["ht=128-rounds=1", "ht=128-rounds=2", "several-rounds", "beyond-prefetch-class-3", "beyond-prefetch-class-4",
                    "empty-read-first", "empty-read-last", "empty-read-between-classes", "65-reads-of-one-class-beside-others",
                    "wavefront-with-mixed-classes", "ragged-read-count"],
    "row_duplicates": ["dup-twice", "dup-thrice-middle", "dup-first-by-last", "dup-d=1", "dup-ht=128-d=96-rounds=1", "dup-ht=128-d=97-rounds=2",
                       "dup-one-round", "dup-several-rounds", "dup-load-1.0", "dup-positions-differ", "dup-across-prefetch-class-3",
                       "dup-across-prefetch-class-4"] + ["dup-class-%d" % q for q in range(5)],
    "row_probes": [key + "-ht=%d" % h for key in ("one-home", "slot-chain-wraps", "dedup-chain-wraps") for h in (16, 128, 1024)] +
                  ["next-free-wraps-ht=128", "next-free-wraps-ht=1024", "global-class-wraps"],
    "row_global": ["global-class-more-reads-than-workgroups", "two-workgroups-take-a-second-read", "second-read-smaller-and-larger-table",
                   "global-class-two-reads-with-duplicates", "global-n=8193", "global-n=16384", "global-n=16385", "load-1.0-ht=16384"],
    "row_limits": ["n=65535", "row_limits_over", "row_limits_order"],
}
WINDOW_KEYS = ["begins-at-first-entry", "begins-31-before", "begins-32-before", "begins-33-before", "ends-31-past", "ends-32-past",
               "ends-33-past", "first-workgroup-long-run", "last-workgroup-run-to-the-end", "run-longer-than-window",
               "run-bounds-left-0-steps", "run-bounds-left-16-steps", "run-bounds-left-bisects-at-17", "run-bounds-right-0-steps",
               "run-bounds-right-16-steps", "run-bounds-right-bisects-at-17", "run-bounds-both-bisect"]
LAYOUT_KEYS = {
    "runs": ["wg%d-%s" % (blk, key) for blk in M.EMIT_BLOCKS for key in WINDOW_KEYS] + ["degree=%d" % d for d in A.RUN_DEGREES] +
            ["both-strands-planted", "place-pass-sorts"],
    "palindromes": ["palindrome-degree=%d" % d for d in (1, 2, 3, 40)] +
                   ["palindrome-last-but-one-not-inline", "inline-same-strand", "inline-opposite-strands", "k=2"],
    "sizes": ["nnz=%d" % n for n in (1, 255, 256, 257, 2048, 4096, 4097)] + ["nkmers=2^%d" % b for b in (1, 8, 12, 20)] +
             ["nkmers=2^%d+1" % b for b in (1, 8, 12, 20)] +
             ["largest-id-in-use", "fewer-nonzeros-than-reads", "place-pass-plain", "place-pass-sorts", "partitioned-place-pass-plain",
              "partitioned-place-pass-sorts"],
    "chunks": ["chunk-none", "chunk-fast", "chunk-search", "chunk-one-entry-with-2-among-63-with-1", "chunk-more-than-64-products",
               "live-entry-last-of-chunk-and-first-of-next", "row-of-64-entries", "row-of-65-entries", "dead-row-between-live-rows"],
    "rowlists": ["round-tot=2n", "round-tot=2n+1", "round-tot=12n", "round-tot=12n+1", "round-L=1", "round-L=4", "round-L=16",
                 "row-of-1025-live-entries", "row-of-2049-live-entries", "rounds-with-different-L", "one-product-entries-in-L=4-round",
                 "one-product-entries-in-L=16-round"],
}


@pytest.mark.parametrize("family", list(ROW_KEYS))
def test_census_rows(family):
    seen = set()
    for name in A.FAMILIES[family]:
        seen |= A.census_rows(A.case(name))
    missing = [key for key in ROW_KEYS[family] if key not in seen]
    print(family, sorted(seen))
    assert not missing, missing


@pytest.mark.parametrize("family", list(LAYOUT_KEYS))
def test_census_layout(family):
    seen = set()
    for name in A.FAMILIES[family]:
        seen |= A.census_layout(A.case(name), oracle_B(name))
    missing = [key for key in LAYOUT_KEYS[family] if key not in seen]
    print(family, sorted(seen))
    assert not missing, missing


def test_sizes_have_the_nonzeros_they_are_for():
    for name in A.FAMILIES["sizes"]:
        c = A.case(name)
        Bc, Br, _ = oracle_B(name)
        assert len(Br) == len(c.tk) == c.design["nnz"]               # (a k-mer appears once per read: no entry merges)


def test_every_family_has_its_keys():
    assert set(ROW_KEYS) | set(LAYOUT_KEYS) | {"degree_limit"} == set(A.FAMILIES)


def test_degree_limit_design():
    """16,383 reads share one k-mer (16,384 in the error case); the products follow from the degrees"""
    for nshare in (16383, 16384):
        c = A.case("degree_%d" % nshare)
        deg = np.bincount(c.tk, minlength=c.nkmers)
        assert sorted(deg) == [2, 3, 5, nshare] and c.design["flops"] == int((deg * (deg - 1) // 2).sum())
        assert c.design["flops"] == nshare * (nshare - 1) // 2 + 1 + 3 + 10
        L = c.layout(oracle_B(c.name))
        assert L.over_degree == (nshare > M.MAX_DEGREE) and int(L.degree.max()) == nshare


@pytest.mark.parametrize("name", ["chunks", "rowlists"])
def test_hub_rows_are_the_designed_ones(name):
    c = A.case(name)
    A.check_hub_rows(c, c.layout(oracle_B(name)))


def test_runs_are_where_the_plan_puts_them():
    c = A.case("runs")
    L = c.layout(oracle_B("runs"))
    heads = L.rank == 0
    assert L.degree[heads].tolist() == c.design["plan"] and L.nnz == c.design["nnz"]
    assert np.array_equal(L.skey[heads], np.arange(len(c.design["plan"])))


@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_mirror_products_equal_oracle(name):
    """the mirror's later-read counts add up to the oracle's products, whole and per partition"""
    c = A.case(name)
    B = oracle_B(name)
    flop, _, _ = O.spgemm(c.seqs, c.nkmers, *B, c.k)
    flop = np.asarray(flop).astype(np.int64)
    assert c.layout(B).products() == int(flop.sum())
    for f in range(3):
        assert c.layout(B, f, 3).products() == int(flop[f::3].sum())


def test_assemble_stats_is_declared_and_bound():
    from bella_amd import _lib
    assert "bella_hip_get_assemble_stats" in open(os.path.join(ROOT, "include", "bella_hip.h")).read()
    assert "bella_hip_get_assemble_stats" in {s[0] for s in _lib.SIGNATURES} and hasattr(_lib.load(), "bella_hip_get_assemble_stats")
