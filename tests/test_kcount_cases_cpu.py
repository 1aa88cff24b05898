"""The k-mer counting cases of bella_testkit/kcount_cases.py without a device: the numpy mirror (bella_testkit/kcount_mirror.py)
against the C oracle on every case and on the synthetic sets of the three parameter sweeps of tests/test_gpu_parity.py -- dictionary
words and counts, the three tuple arrays and the number of distinct words, all exactly -- then the geometry each case was built
for, read back from the mirror's description, and a census: the case tables together hold every tile, group, counter, table, ring
and pass geometry that tests/test_kcount_edges_gpu.py is there to run.  The census counts tags; it does not trust the builders."""
import numpy as np
import pytest

import _oracle as O
from bella_testkit import kcount_cases as KC
from bella_testkit import kcount_mirror as M
from bella_testkit import synth


def oracle_count(c):
    return O.count_kmers(c.rs.seqs(), c.k, c.lower, c.upper, c.mode == 1, c.window if c.mode == 2 else 0)


def mirror_equals_oracle(cd, exp, what):
    codes, counts, tk, tr, tp, nd = exp
    assert (len(cd.codes), len(cd.t_kmer), cd.ndistinct) == (len(codes), len(tk), nd), what
    for name, a, b in (("codes", cd.codes, codes), ("counts", cd.counts, counts), ("t_kmer", cd.t_kmer, tk), ("t_read", cd.t_read, tr),
                       ("t_pos", cd.t_pos, tp)):
        assert np.array_equal(a, b), (what, name)


@pytest.mark.parametrize("family", list(KC.FAMILIES))
def test_mirror_equals_oracle_and_every_case_has_its_geometry(family):
    cases = KC.family(family)
    assert len({c.name for c in cases}) == len(cases)
    reads = tiles = npass = 0
    for c in cases:
        d = c.describe()
        mirror_equals_oracle(d["counted"], oracle_count(c), (family, c.name))
        have = KC.tags(c)
        assert all(w in have for w in c.want), (family, c.name, [w for w in c.want if w not in have])
        assert c.want, (family, c.name)
        reads, tiles, npass = reads + c.rs.nreads, tiles + sum(d["tiles"]), npass + len(d["passes"])
    print("%s: %d cases, %d reads, %d tiles, %d passes" % (family, len(cases), reads, tiles, npass))


SWEEPS = [(0, dict(nreads=70, read_len=900, coverage=12.0, err=0.1, seed=11),
           [(17, 0, 2, 8), (11, 0, 2, 4), (32, 0, 2, 8), (3, 0, 2, 65535), (5, 0, 3, 60000), (21, 0, 2, 2)]),
          (1, dict(nreads=60, read_len=1200, coverage=10.0, err=0.01, seed=13, mix=(1 / 3, 1 / 3, 1 / 3)),
           [(17, 0, 2, 8), (6, 0, 2, 60000), (11, 0, 2, 30), (21, 0, 2, 4), (32, 0, 2, 8), (7, 0, 3, 65535)]),
          (2, dict(nreads=60, read_len=1200, coverage=10.0, err=0.02, seed=29, mix=(1 / 3, 1 / 3, 1 / 3)),
           [(17, 10, 2, 8), (15, 1, 2, 30), (21, 50, 2, 8), (32, 7, 2, 8), (5, 3, 2, 65535), (17, 3000, 2, 8)])]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_mirror_equals_oracle_on_the_sets_of_the_parameter_sweeps(mode):
    _, kw, pars = SWEEPS[mode]
    rs = synth.make_reads(**kw)
    seqs = rs.seqs()
    for k, window, lower, upper in pars:
        exp = O.count_kmers(seqs, k, lower, upper, mode == 1, window)
        mirror_equals_oracle(M.count(rs, k, lower, upper, mode, window), exp, (mode, k, window, lower, upper))


def test_mirror_hashes_equal_the_oracles():
    rng = np.random.default_rng(5)
    w = rng.integers(0, 1 << 63, 200, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 200, dtype=np.uint64)
    got = M.kmer_hash(w)
    assert [int(x) for x in got] == [O.lib().oracle_kmer_hash(int(x)) for x in w]
    # splitmix64's published test vector: the finaliser of the first three states from seed 0
    g = 0x9e3779b97f4a7c15
    assert [int(x) for x in M.mix64(np.asarray([g, 2 * g % 2 ** 64, 3 * g % 2 ** 64], np.uint64))] == \
           [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]


def test_plan_at_the_limits_of_the_fast_path():
    for k, limit, gb in ((25, 16384, 2), (24, 65536, 0), (31, 4, 0), (29, 64, 2)):
        fast, pb, g = M.plan(limit, k, 0)
        assert fast and 2 * k + pb == 64 and g == gb
        assert M.plan(limit + 1, k, 0) == (False, 0, 0)
        assert M.plan(limit, k, 2)[0] and not M.plan(limit, k, 1)[0] and not M.plan(limit, k, 0, M.DEBUG_LOOKUP)[0]
    assert [M.plan(1000, k, 0)[2] for k in (4, 5, 6, 13, 16, 17, 21)] == [0, 2, 0, 2, 0, 2, 2]
    assert not M.plan(1000, 32, 0)[0]


def test_passes_under_a_budget():
    hist = np.zeros(256, np.int64)
    hist[[0, 20, 40, 255]] = [306, 5000, 456, 3]
    assert M.passes(hist, 400, 0, int(hist.sum())) == [(0, 20, 306), (20, 21, 5000), (21, 40, 0), (40, 41, 456), (41, 256, 3)]
    assert M.passes(hist, 0, 0, int(hist.sum())) == [(0, 256, int(hist.sum()))]
    assert M.passes(hist, 0, 2, int(hist.sum())) == [(0, 256, int(hist.sum()))]             # one pass, sized by the histogram
    assert M.passes(hist, 5500, 0, int(hist.sum())) ==[(0, 40, 5306), (40, 256, 459)]


def test_the_case_tables_hold_every_geometry():
    """census over (family, k, mode, debug bit 14, tag)"""
    seen = set()
    by_case = {}
    for fam in KC.FAMILIES:
        for c in KC.family(fam):
            tg = KC.tags(c)
            by_case[(fam, c.name)] = tg
            for t in tg:
                seen.add((fam, c.k, c.mode, bool(c.debug), t))
    need = []
    for k in (17, 16, 13):
        te = ["total:%d" % n for n in KC.TOTALS] + ["head:e%d" % e for e in KC.EDGE_E] + ["head:e%d:inner-tile" % e for e in KC.EDGE_E]
        te += ["end:inner:-1", "end:inner:+0", "end:inner:+1", "end:last:-1", "end:last:+0", "bisect:zero-extra", "tile-start:fresh",
               "tile-start:continued", "tile:last-partial"]
        need += [("tile_edges", k, 0, False, t) for t in te]
    for k in (17, 13, 5):
        for m in range(1, 16):
            need += [("masks", k, 0, False, "mask:k%d:%d:%s" % (k, m, x)) for x in ("absent", "low", "high", "planes>=2", "planes=7", "a0", "a63")]
    need += [("dense", 17, 0, False, t) for t in ("rec:1024", "rec:1023", "rec:1024:twice-in-a-row")]
    lr = ["big:v%d:65538:u8" % v for v in (0, 2, 3)] + ["big:next-head:e0", "big:next-head:e1", "big:whole-tiles-inside>=2", "tiles:headless>=2", "head:e2047"]
    for n in (65535, 65536, 65537, 65538):
        lr += ["big:v2:%d:u65535" % n, "big:%d:reliable-neighbour" % n]
    need += [("long_runs", 17, 0, False, t) for t in lr]
    for mode in (1, 2):
        for n in (65535, 65536, 65537, 65538):
            need += [("saturation", 17, mode, False, "sat:m%d:%d:u%d:%s" % (mode, n, u, x)) for u, x in
                     ((65535, "reliable"), (65534, "not-reliable"), (65535, "with-neighbour"), (65534, "with-neighbour"))]
    for k, limit in ((25, 16384), (24, 65536), (31, 4), (29, 64)):
        need += [("fast_limit", k, 0, False, t) for t in ("plan:k%d:n%d:fast" % (k, limit), "plan:k%d:n%d:lookup" % (k, limit + 1), "key:bit63",
                                                           "positions:field-full", "tuple:last-position")]
    for k, mode, dbg in ((17, 0, True), (32, 0, False), (17, 1, False)):
        need += [("lookup", k, mode, dbg, "dict:%d" % n) for n in (511, 512, 513, 1024, 1025)]
        need += [("lookup", k, mode, dbg, t) for t in ("table:load-half", "table:last-slot>=4", "table:last-slot-misses>=4", "path:lookup")]
    need.append(("lookup", 32, 1, False, "table:all-T-left-out"))
    for k in (17, 5):
        for w in (1, 2, 3, 10, 39, 40, 41):
            need += [("minimizer_ring", k, 2, False, "ring:k%d:w%d:r%d" % (k, w, r)) for r in (1, 63, 64, 65, 129)]
        need += [("minimizer_ring", k, 2, False, t) for t in ("ring:full", "ring:w-nk:-1", "ring:w-nk:+0", "ring:w-nk:+1", "ring:nothing-sampled",
                                                               "ring:sampled", "ring:full-beside-short")]
    for mode, how in ((2, "one-pass"), (2, "passes"), (0, "passes")):
        need += [("emit_chunks", 17, mode, False, "emit:%d:m%d:%s" % (n, mode, how)) for n in (1023, 1024, 1025, 2048, 2049)]
    need += [("multi_pass", 17, 0, False, t) for t in ("passes>=3", "pass:over-budget", "pass:zero-between", "pass:ends-after-big-bin", "pass:bins-0-255")]
    missing = [n for n in need if n not in seen]
    assert not missing, missing[:20]
    # the periodic cases with a window the reads can fill do fill the ring
    for c in KC.family("minimizer_ring"):
        if c.window <= 10:
            assert "ring:full" in by_case[("minimizer_ring", c.name)], c.name
    # several passes AND the edge, in one case
    multi = [tg for (fam, _), tg in by_case.items() if fam == "multi_pass"]
    for t in ("head:e2047", "head:e2016", "end:inner:+0", "mask:k17:15:low", "mask:k17:7:planes=7", "big:v2:65538:u8"):
        assert any(t in tg and "passes>=3" in tg for tg in multi), t
    names = {c.name for c in KC.family("small_k")}
    assert names >= {"all-k%d" % k for k in range(1, 7)} | {"syncmers-k6", "syncmers-k7"} | \
        {"minimizers-k%d-w%d-len+%d" % (k, w, x) for k in range(1, 6) for w in (1, 2) for x in (1, 2)}
    for c in KC.family("small_k"):
        if c.name.startswith("all-k"):
            assert c.rs.nreads and len(np.unique(c.rs.lengths)) == 1 and int(c.rs.lengths[0]) == c.k
    print("%d cases, %d tags required, %d distinct tags seen" % (len(by_case), len(need), len(seen)))


def test_count_stats_is_declared_and_bound():
    import os
    from bella_amd import _lib
    from conftest import ROOT
    assert "bella_hip_get_count_stats" in open(os.path.join(ROOT, "include", "bella_hip.h")).read()
    assert "bella_hip_get_count_stats" in {s[0] for s in _lib.SIGNATURES} and hasattr(_lib.load(), "bella_hip_get_count_stats")
