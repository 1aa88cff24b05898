"""GPU tests of the stage state of the assembly stages: which results a context holds after every call is what
one table of dependencies predicts; and the kernels the tip and the bubble rounds share, on graphs whose edge count is a multiple of
the block size (the scan's sentinel element keep[m] is then the first thread of a block of its own)."""
import ctypes as C

import numpy as np
import pytest

from bella_amd import Engine, _lib
from bella_testkit import bubble_mirror as B
from bella_testkit import graph_mirror as G
from bella_testkit import synth
from bella_testkit import unitig_mirror as U

pytestmark = pytest.mark.gpu

STATE, BAD_ARG = -7, -3


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- the rule as a table -----------------------------------------------------------------------------------------------------------
# the model: what is built from what.  A stage that changes takes along everything built from it; one that is dropped goes itself too.
BUILT_FROM = {"trim": ("records",), "graph": ("records", "trim"), "unitigs": ("graph",), "polish": ("unitigs", "pile"), "cons": ("pile",)}
FIRST = {"graph": "bella_hip_graph_build first", "trim": "bella_hip_graph_trim first", "unitigs": "bella_hip_graph_unitigs first",
         "polish": "bella_hip_graph_polish_unitigs first"}


def changed(valid, stage):
    for s, parts in BUILT_FROM.items():
        if stage in parts:
            drop(valid, s)


def drop(valid, stage):
    valid.discard(stage)
    changed(valid, stage)


def made(valid, stage):
    drop(valid, stage)
    valid.add(stage)


def _getters(eng):
    lib, h = eng.lib, eng.h

    def stats(fn, struct):
        st = struct()
        return lambda: fn(h, C.byref(st), C.sizeof(st))
    return {
        "graph": ("graph", lambda: lib.bella_hip_graph_get(h, None, None, None, None, None)),
        "graph_stats": ("graph", stats(lib.bella_hip_graph_get_stats, _lib.GraphStats)),
        "graph_removed": ("graph", lambda: lib.bella_hip_graph_get_removed(h, None)),
        "bubble_stats": ("graph", stats(lib.bella_hip_graph_get_bubble_stats, _lib.BubbleStats)),
        "unitig_stats": ("graph", stats(lib.bella_hip_graph_get_unitig_stats, _lib.UnitigStats)),
        "get_trim": ("trim", lambda: lib.bella_hip_graph_get_trim(h, None)),
        "get_trim_stats": ("trim", stats(lib.bella_hip_graph_get_trim_stats, _lib.TrimStats)),
        "get_unitigs": ("unitigs", lambda: lib.bella_hip_graph_get_unitigs(h, *[None] * 7)),
        "get_unitig_bases": ("unitigs", lambda: lib.bella_hip_graph_get_unitig_bases(h, None, None)),
        "get_polished": ("polish", lambda: lib.bella_hip_graph_get_polished(h, *[None] * 5)),
        "get_polish_stats": ("polish", stats(lib.bella_hip_graph_get_polish_stats, _lib.PolishStats)),
    }


def test_every_call_drops_what_the_table_says(eng):
    starts, lens, strands, recs = G.truth_chain(60)
    rs = synth.ReadSet.from_strings(B.dummy_seqs(lens))
    lib, h = eng.lib, eng.h
    bad = recs[:1].copy()
    bad["rid"] = bad["cid"]
    no_depth = _lib.GraphTrimParams(C.sizeof(_lib.GraphTrimParams), 0, 500, 1000)
    one = np.zeros((int(lens[0]), 9), np.uint32)
    one[5, 0] = 1

    def records(v):
        changed(v, "records")

    def graph_changed(v):
        changed(v, "graph")

    def pile_changed(v):
        changed(v, "pile")

    def untrim(v):
        if "trim" in v:
            drop(v, "trim")

    def reload(v):
        v.clear()

    nothing = lambda v: None
    make = lambda stage: (lambda v: made(v, stage))
    build, trim, unitigs, polish = (eng.graph_build, make("graph")), (eng.graph_trim, make("trim")), (eng.graph_unitigs, make("unitigs")), \
        (eng.graph_polish_unitigs, make("polish"))
    script = [
        ("set_reads", lambda: eng.set_reads(rs), reload),
        ("add_overlaps", lambda: eng.graph_add_overlaps(recs), records),
        ("build", *build),
        ("trim", *trim),                                              # a trim drops the graph
        ("build", *build),
        ("clean rounds=0", lambda: eng.graph_clean(tip_rounds=0), graph_changed),
        ("unitigs", *unitigs),
        ("pop rounds=0", lambda: eng.graph_pop_bubbles(bubble_rounds=0), graph_changed),
        ("unitigs", *unitigs),
        ("pileup_reset before polish", eng.pileup_reset, make("pile")),
        ("polish", *polish),
        ("pileup_reset after polish", eng.pileup_reset, make("pile")),
        ("polish", *polish),
        ("trim refused", lambda: lib.bella_hip_graph_trim(h, C.byref(no_depth)), nothing, BAD_ARG),
        ("add_overlaps refused", lambda: lib.bella_hip_graph_add_overlaps(h, bad.ctypes.data, 1), nothing, BAD_ARG),
        ("clean", eng.graph_clean, graph_changed),
        ("unitigs", *unitigs),
        ("polish", *polish),
        ("add_pileup", lambda: eng.add_pileup(0, 1, one), pile_changed),
        ("polish", *polish),
        ("pop", eng.graph_pop_bubbles, graph_changed),
        ("unitigs", *unitigs),
        ("polish", *polish),
        ("unitigs again", *unitigs),                                  # new unitigs drop the polish
        ("polish", *polish),
        ("build again", *build),                                      # keeps the trim
        ("unitigs", *unitigs),
        ("untrim with a trim", eng.graph_untrim, untrim),
        ("untrim without one, no graph", eng.graph_untrim, untrim),
        ("build", *build),
        ("unitigs", *unitigs),
        ("untrim without one, a graph", eng.graph_untrim, untrim),   # nothing happens: the graph stays
        ("polish", *polish),
        ("add_overlaps of nothing", lambda: eng.graph_add_overlaps(recs[:0]), records),
        ("trim", *trim),
        ("build", *build),
        ("unitigs", *unitigs),
        ("polish", *polish),
        ("graph_reset", eng.graph_reset, records),
        ("add_overlaps", lambda: eng.graph_add_overlaps(recs), records),
        ("trim", *trim),
        ("build", *build),
        ("unitigs", *unitigs),
        ("polish", *polish),
        ("set_reads again", lambda: eng.set_reads(rs), reload),
    ]
    getters = _getters(eng)
    valid = set()
    seen = set()
    for step, (label, call, effect, *want) in enumerate(script):
        rc = call()
        assert (rc if isinstance(rc, int) else 0) == (want[0] if want else 0), (step, label, rc)
        effect(valid)
        where = "after step %d (%s), model %s" % (step, label, sorted(valid))
        for name, (stage, get) in getters.items():
            rc = get()
            assert rc == (0 if stage in valid else STATE), (name, rc, where)
            if rc:
                assert lib.bella_hip_last_error(h).decode() == FIRST[stage], (name, where)
        n = C.c_uint64(99)
        assert lib.bella_hip_graph_get_overlaps(h, None, C.byref(n)) == 0, where      # always answers
        seen.add(frozenset(valid & set(FIRST)))
    assert len(seen) >= 8                                             # (the script walks through that many different states)


# ---- the round kernels at a block boundary -----------------------------------------------------------------------------------------
def _load(eng, y):
    lens, recs, ids, _ = y.build()
    eng.set_reads(synth.ReadSet.from_strings(B.dummy_seqs(lens)))
    eng.graph_add_overlaps(recs)
    eng.graph_build()
    m = G.build(recs, lens)
    off, e, cont = eng.graph()
    assert len(e) == 256 and len(e) % 256 == 0
    assert np.array_equal(off, m["offsets"]) and e.tobytes() == m["edges"].tobytes() and np.array_equal(cont, m["contained"])
    return m


def _graph_is(eng, g, contained):
    off, e, cont = eng.graph()
    assert np.array_equal(off, g["offsets"]) and e.tobytes() == g["edges"].tobytes() and np.array_equal(cont, contained)
    assert np.array_equal(eng.graph_removed(), g["removed"])


def test_a_tip_round_over_exactly_one_block_of_edges(eng):
    y = B.Layout()
    y.path(["m%d" % i for i in range(128)])
    y.link("m60", "t0", 2500)
    m = _load(eng, y)
    c = U.clean(m["offsets"], m["edges"], m["contained"])
    eng.graph_clean()
    _graph_is(eng, c, m["contained"])
    st = eng.unitig_stats()
    assert (st["reads_removed"], st["edges_removed"], st["reads_per_round"]) == (1, 2, [1, 0])
    assert int(c["removed"].sum()) == 1 and len(c["edges"]) == 254


def test_a_bubble_round_over_exactly_one_block_of_edges(eng):
    y = B.Layout()
    y.path(["m%d" % i for i in range(125)])
    y.path(["m13", "a0", "a1", "a2", "m16"], 1500)
    m = _load(eng, y)
    r = B.pop(m["offsets"], m["edges"], m["contained"], None)
    eng.graph_pop_bubbles()
    _graph_is(eng, r, m["contained"])
    st = eng.bubble_stats()
    assert (st["reads_removed"], st["edges_removed"]) == (2, 6)
    assert int(r["removed"].sum()) == 2 and len(r["edges"]) == 250
