"""The X-drop kernels on the sets of bella_testkit/xdrop_cases.py (run with `-m gpu` on an MI355X): every field of every pair against the
oracle, under every statement of the kernel -- one launch in sorted order, slices, pair order, the scalar statement -- and under
the slices cut into classes and into batches.  tests/test_xdrop_cases_cpu.py shows what each set holds: extensions that drop, end
or enter Phase 4 on a chosen step around a launch boundary of the sliced kernel, flank lengths around the window sizes, reads at the
edges of the packed array, every k and X, more than 4,096 survivors of four launches, more extensions than a batch.  No tolerance
and no sample: a failure names the configuration and the pair's label."""
import contextlib

import numpy as np
import pytest

from bella_amd import BellaPars, Engine
from bella_amd.api import BellaHipError
from bella_testkit import synth
from bella_testkit import xdrop_cases as XC
from test_xdrop_cases_cpu import FIELDS, oracle_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def tuned(eng, **values):
    try:
        for what, v in values.items():
            eng.set_tuning(what, v)
        yield
    finally:
        for what in values:
            eng.set_tuning(what)


def pars_of(cs):
    return BellaPars(kmerSize=cs.k, xDrop=cs.X, errorRate=cs.err)


def table(alns):
    return np.stack([alns[f].astype(np.int64) for f in FIELDS], 1)


def same_as_oracle(cs, alns, config, reps=1):
    got, exp = table(alns), np.tile(oracle_records(cs), (reps, 1))
    assert got.shape == exp.shape, (cs.name, config)
    for n in np.flatnonzero((got != exp).any(1)):
        m = n % len(cs.seeds)
        raise AssertionError("%s under %s: pair %d %r seed %r: got %r, oracle %r (%s)"
                             % (cs.name, config, m, cs.labels[m], cs.seeds[m], got[n].tolist(), exp[n].tolist(), ", ".join(FIELDS)))
    return len(got)


def configurations(cs):
    """name -> (tuning values, how often the seeds are repeated): classes need 1,024 extensions in a batch, so a small set runs
    several times over in one call; the batches cut the extensions into three, the last one partial"""
    n = len(cs.seeds)
    return {
        "variant 0": (dict(xdrop_variant=0), 1),
        "variant 1": (dict(xdrop_variant=1), 1),
        "variant 2": (dict(xdrop_variant=2), 1),
        "variant 3": (dict(xdrop_variant=3), 1),
        "variant 1 in classes": (dict(xdrop_variant=1, xdrop_class_min=1024), -(-512 // n)),
        "variant 1 in batches": (dict(xdrop_variant=1, xdrop_batch=2 * n // 3 + 1), 1),
    }


def every_configuration(eng, cs):
    eng.set_reads(cs.rs)
    sd = cs.seed_array()
    compared = {}
    for name, (tuning, reps) in configurations(cs).items():
        with tuned(eng, **tuning):
            alns = eng.xdrop_batch(np.tile(sd, reps), pars_of(cs))
        compared[name] = same_as_oracle(cs, alns, name, reps)
    print("%s: pairs compared per configuration %r" % (cs.name, compared))


SMALL = {"drop": XC.drop_set, "end": XC.end_set, "taildrop": XC.tail_drop_set, "kept100": lambda: XC.kept_set(100),
         "kept127": lambda: XC.kept_set(127), "early": XC.early_set, "flank": XC.flank_set, "place0": lambda: XC.place_set(0),
         "place1": lambda: XC.place_set(1), "place15": lambda: XC.place_set(15)}


@pytest.mark.parametrize("name", list(SMALL))
def test_edge_sets_under_every_configuration(eng, name):
    cs = SMALL[name]()
    assert cs.name == name
    every_configuration(eng, cs)


@pytest.mark.parametrize("k", XC.KS)
@pytest.mark.parametrize("X", XC.XS)
def test_mixed_set_under_every_k_and_x(eng, k, X):
    every_configuration(eng, XC.mixed_set(k, X))


SURVIVOR_RUNS = {
    "one batch, no classes": dict(xdrop_variant=1),
    "classes": dict(xdrop_variant=1, xdrop_class_min=1024),
    "batches of 2000": dict(xdrop_variant=1, xdrop_batch=2000),                      # 2,000 + 2,000 + 900
    "batches of 2000, classes": dict(xdrop_variant=1, xdrop_batch=2000, xdrop_class_min=1024),   # (the last batch is below the floor of the classes)
    "batches of 4096": dict(xdrop_variant=1, xdrop_batch=4096),                      # one full batch and a partial one
    "batches of 4096, classes": dict(xdrop_variant=1, xdrop_batch=4096, xdrop_class_min=1024),
    "batch knob 0 = the rule": dict(xdrop_variant=1, xdrop_batch=0),
    "variant 0": dict(xdrop_variant=0),
    "variant 2": dict(xdrop_variant=2),
    "variant 3": dict(xdrop_variant=3),
}


@pytest.mark.parametrize("run", list(SURVIVOR_RUNS))
def test_survivor_set(eng, run):
    """4,900 extensions, 4,700 of them alive after four launches: the survivor count that comes back every fourth slice, the
    compaction of the 200 that end at once, state slots and lists reused from batch to batch, classes within a batch"""
    cs = XC.survivor_set()
    eng.set_reads(cs.rs)
    with tuned(eng, **SURVIVOR_RUNS[run]):
        alns = eng.xdrop_batch(cs.seed_array(), pars_of(cs))
    assert same_as_oracle(cs, alns, run) == 2450


def test_two_calls_on_one_engine(eng):
    """the survivor set, then three pairs: the result buffer is cleared per call, state and lists are reused"""
    for cs in (XC.survivor_set(), XC.tiny_set(), XC.survivor_set()):
        eng.set_reads(cs.rs)
        same_as_oracle(cs, eng.xdrop_batch(cs.seed_array(), pars_of(cs)), "call on " + cs.name)


def test_through_pair_records_with_x60(eng):
    """the mixed set's reads assembled and overlapped as usual: the seeds are the ones the SpGEMM picks, and align_pairs runs with an X
    it was never run with"""
    cs = XC.mixed_set(17, 60)
    rs = cs.rs
    t = synth.count_and_tuples(rs, 17, 2, 8)
    eng.set_reads(rs)
    eng.assemble_tuples(17, t.nkmers, t.kmer, t.read, t.pos)
    pars = pars_of(cs)
    eng.overlap(pars)
    pairs, _, _ = eng.get_pairs(ext=False)
    assert len(pairs) >= 150
    seeds = [(int(p["rid"]), int(p["cid"]), int(p["seedH"]), int(p["seedV"])) for p in pairs]
    via = XC.CaseSet("mixed-pairs-x60", 17, 60, cs.seqs, seeds, [dict(event="pair record")] * len(seeds))
    for variant in (1, 0, 2, 3):
        with tuned(eng, xdrop_variant=variant):
            npass = eng.align_pairs(pars)
            alns = eng.get_alignments()
        same_as_oracle(via, alns, "align_pairs, variant %d" % variant)
        assert npass == int(oracle_records(via)[:, FIELDS.index("passed")].sum())
    with tuned(eng, xdrop_class_min=1024, xdrop_batch=len(seeds)):
        eng.align_pairs(pars)
        same_as_oracle(via, eng.get_alignments(), "align_pairs in two batches")


def test_xdrop_above_127_is_rejected_by_both_entries(eng):
    cs = XC.tiny_set()
    rs = cs.rs
    t = synth.count_and_tuples(rs, 17, 2, 8)
    eng.set_reads(rs)
    eng.assemble_tuples(17, t.nkmers, t.kmer, t.read, t.pos)
    eng.overlap(BellaPars(kmerSize=17))
    sd = cs.seed_array()
    with pytest.raises(BellaHipError) as by_pairs:
        eng.align_pairs(BellaPars(kmerSize=17, xDrop=128))
    with pytest.raises(BellaHipError) as by_seeds:
        eng.xdrop_batch(sd, BellaPars(kmerSize=17, xDrop=128))
    assert by_seeds.value.code == by_pairs.value.code == -3 and str(by_seeds.value) == str(by_pairs.value) and "127" in str(by_seeds.value)
    same_as_oracle(cs, eng.xdrop_batch(sd, pars_of(cs)), "after the rejected call")               # the context keeps working
    same_as_oracle(XC.CaseSet("tiny-x127", 17, 127, cs.seqs, cs.seeds, cs.labels), eng.xdrop_batch(sd, BellaPars(kmerSize=17, xDrop=127)), "X = 127")
    assert len(eng.xdrop_batch(sd, BellaPars(kmerSize=17, xDrop=128), exact=True)) == 3             # LOGAN's scores are not int8
