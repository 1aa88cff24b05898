"""GPU tests of the traced alignments below their covering band: every field of every record and every op
word of bella_hip_trace_batch / _trace_pairs against the banded mirror (bella_testkit/trace_mirror.py: trace_expect_banded), which
is exact at any band -- score, end points, counters, the band the pair ended with, its doublings, and the path op for op.  The
hand-made list (bella_testkit/trace_cases.py) reaches the four DP kernels with windows that slide past their band, both band edges,
every widening step and the bookkeeping of bella_trace_stats; two sets of real shape run at the default band."""
import collections
import multiprocessing as mp
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib
from bella_testkit import synth
from bella_testkit import trace_cases as T
from bella_testkit import trace_mirror as M

pytestmark = pytest.mark.gpu

FIELDS = ("score", "tbegH", "tendH", "tbegV", "tendV", "n_eq", "n_x", "n_ins", "n_del", "band", "widened")


@pytest.fixture(scope="module")
def listed():
    """the case list, its reads, its expectation at every first band -- computed once, never changed"""
    cases = T.build_cases()
    expect = T.expectations(cases)
    T.check_coverage(T.coverage(cases, expect))            # the list still reaches what it is for: it cannot quietly degenerate
    return cases, T.read_set(cases), expect


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _compare(tr, ops, expect, label):
    """records and op words against [(record, ops, steps)]; the records' runs tile the op array (a repeated pair's runs come after
    those of the pairs that finished before it, so the order is the order of finishing, not of the list)"""
    assert len(tr) == len(expect)
    for q, (rec, want, _) in enumerate(expect):
        got = {f: int(tr[q][f]) for f in FIELDS}
        assert got == rec, (label, q, got, rec)
        at = int(tr[q]["op_off"])
        assert int(tr[q]["nops"]) == len(want), (label, q)
        assert np.array_equal(ops[at:at + len(want)], want), (label, q, M.cigar(ops[at:at + len(want)])[:300], M.cigar(want)[:300])
    order = np.argsort(tr["op_off"], kind="stable")
    ends = tr["op_off"][order] + tr["nops"][order]
    assert int(tr["op_off"][order[0]]) == 0 and np.array_equal(tr["op_off"][order][1:], ends[:-1]) and int(ends[-1]) == len(ops)


def _classes(expect):
    """side DPs per kernel class (256, 512, 1,024, wider) and doublings, from the mirror's steps"""
    dps = collections.Counter(min(b, 2048) for _, _, steps in expect for s in steps for b, _ in s)
    return [dps[b] for b in (256, 512, 1024, 2048)], sum(r["widened"] for r, _, _ in expect)


@pytest.mark.parametrize("band0", T.BAND0S)
def test_hand_made_list_equals_the_banded_mirror(eng, listed, band0):
    """one trace_batch call over the whole list (all kernel classes in one batch): records, ops and the call's statistics"""
    cases, rs, expect = listed
    exp = expect[band0]
    eng.set_reads(rs)
    seeds = np.zeros(len(cases), _lib.SEED_DT)
    alns = np.zeros(len(cases), _lib.ALN_DT)
    for q, c in enumerate(cases):
        seeds[q] = (2 * q, 2 * q + 1, c.seedH, c.seedV)
        for f in ("begH", "endH", "begV", "endV", "strand"):
            alns[q][f] = c.aln[f]
        alns[q]["passed"] = 1
    assert seeds["rid"][0] == 0 and seeds["cid"][-1] == rs.nreads - 1
    tr, ops = eng.trace_batch(seeds, alns, BellaPars(kmerSize=T.K), band0=band0)
    st = eng.trace_stats()
    dps, doublings = _classes(exp)
    print("TRACE banded list, first band %d: %d pairs, side DPs at 256 / 512 / 1,024 / wider: %s, doublings %d, repeated pairs %d"
          % (M.first_band(band0), len(cases), dps, doublings, T.bookkeeping(exp)["repeated_pairs"]))
    _compare(tr, ops, exp, "band0 %d" % band0)
    book = T.bookkeeping(exp)
    assert (st.widened_extensions, st.repeated_pairs, st.extensions) == (book["widened_extensions"], book["repeated_pairs"], book["extensions"])
    assert st.band0 == M.first_band(band0) and st.pairs == len(cases) and st.ops == len(ops)


_JOBS = None


def _mirror_job(q):
    H, V, sh, sv, k, a = _JOBS[q]
    return M.trace_expect_banded(H, V, sh, sv, k, a, 0)


def _mirror(jobs):
    global _JOBS
    _JOBS = jobs
    # (forked workers inherit the parent's device file descriptors: 12 of them + the parent stay clear of a limit of 16 such processes)
    with mp.get_context("fork").Pool(min(12, os.cpu_count() or 1)) as pool:
        return pool.map(_mirror_job, range(len(jobs)), chunksize=8)


def _real_shape(eng, seqs, pairs, alns, pars, k, pick, label):
    """trace_pairs at the default band; the pairs of `pick` against the mirror"""
    tr, ops = eng.trace_pairs(pars)
    passed = np.flatnonzero(alns["passed"])
    assert int((tr["nops"] > 0).sum()) == len(passed) and int(tr["nops"].sum()) == len(ops)
    jobs = [(seqs[int(pairs[n]["rid"])], seqs[int(pairs[n]["cid"])], int(pairs[n]["seedH"]), int(pairs[n]["seedV"]), k,
             {f: int(alns[n][f]) for f in ("begH", "endH", "begV", "endV", "strand")}) for n in pick]
    exp = _mirror(jobs)
    dps, doublings = _classes(exp)
    print("TRACE banded %s: %d pairs compared, side DPs at 256 / 512 / 1,024 / wider: %s, doublings %d" % (label, len(pick), dps, doublings))
    for n, (rec, want, _) in zip(pick, exp):
        got = {f: int(tr[n][f]) for f in FIELDS}
        assert got == rec, (label, n, got, rec)
        o = ops[int(tr[n]["op_off"]):int(tr[n]["op_off"]) + int(tr[n]["nops"])]
        assert np.array_equal(o, want), (label, n, M.cigar(o)[:300], M.cigar(want)[:300])
    return exp


@pytest.mark.parametrize("golden", ["toy120"], indirect=True)
def test_golden_set_default_band_equals_the_banded_mirror(eng, golden):
    """toy120, every passed pair, as the product traces them"""
    g = golden
    eng.set_reads(g.rs)
    eng.assemble_tuples(g.k, g.nkmers, g.tk, g.tr, g.tp)
    pars = BellaPars(kmerSize=g.k, errorRate=g.err)
    eng.overlap(pars)
    pairs, _, _ = eng.get_pairs()
    eng.align_pairs(pars)
    alns = eng.get_alignments()
    passed = np.flatnonzero(alns["passed"]).tolist()
    assert len(passed) > 1000
    exp = _real_shape(eng, g.seqs, pairs, alns, pars, g.k, passed, "toy120")
    st = eng.trace_stats()
    assert st.pairs == len(passed) and st.widened_extensions == sum(r["widened"] for r, _, _ in exp)
    assert st.extensions == 2 * sum(len(s[0]) for _, _, s in exp) and st.repeated_pairs == sum(len(s[0]) - 1 for _, _, s in exp)
    assert st.band0 == M.first_band(0) == 256


def test_synthetic_3kb_reads_default_band_equals_the_banded_mirror(eng):
    """300 reads of 3 kb at 15 % error: a fixed-seed sample of 48 passed pairs"""
    rs = synth.make_reads(300, read_len=3000, err=0.15, seed=33)
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    pairs, _, _ = eng.get_pairs()
    eng.align_pairs(pars)
    alns = eng.get_alignments()
    passed = np.flatnonzero(alns["passed"])
    assert len(passed) >= 48
    pick = sorted(np.random.default_rng(34).choice(passed, 48, replace=False).tolist())
    _real_shape(eng, rs.seqs(), pairs, alns, pars, 17, pick, "synthetic 300 x 3 kb")
