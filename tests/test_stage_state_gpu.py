"""GPU tests of the stage state of the pipeline's stages: which results a context holds after every call is what
one table of dependencies predicts; and the kernels the tip and the bubble rounds share, on graphs whose edge count is a multiple of
the block size (the scan's sentinel element keep[m] is then the first thread of a block of its own)."""
import ctypes as C

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib
from bella_testkit import bubble_mirror as B
from bella_testkit import graph_mirror as G
from bella_testkit import synth
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import run_ranks

pytestmark = pytest.mark.gpu

STATE, BAD_ARG = -7, -3


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


# ---- the rule as a table -----------------------------------------------------------------------------------------------------------
# the model: what is built from what.  A stage that changes takes along everything built from it; one that is dropped goes itself too.
BUILT_FROM = {"tuples": ("reads",), "panel": ("reads",), "matrix": ("reads",), "pairs": ("matrix",), "alns": ("pairs",), "traces": ("alns",),
              "batch_ops": (), "trim": ("records", "reads"), "graph": ("records", "trim", "reads"), "unitigs": ("graph",),
              "polish": ("unitigs", "pile"), "pile": ("reads",), "cons": ("pile",)}
FIRST = {"graph": "bella_hip_graph_build first", "trim": "bella_hip_graph_trim first", "unitigs": "bella_hip_graph_unitigs first",
         "polish": "bella_hip_graph_polish_unitigs first"}
FRONT_FIRST = {"reads": "set_reads first", "tuples": "count_kmers first", "panel": "assemble_panel first", "matrix": "set_B / assemble_tuples first",
               "pairs": "overlap first", "alns": "align_pairs first", "traces": "trace_pairs first", "batch_ops": "trace_batch first"}


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


# ---- the stages before the graph: reads -> tuples -> panel / matrix -> pairs -> alignments -> traces ----------------------------------
READS_40 = dict(nreads=40, read_len=1500, coverage=10.0, err=0.15, seed=3)        # 62,586 bases; k = 17, 2..8: 1,584 reliable k-mers,
K, LOWER, UPPER = 17, 2, 8                                                         # 3,644 tuples, 316 candidate pairs
ROOM = 4096                                                                        # alignments / trace runs the getters' buffers hold


def _front_getters(eng):
    lib, h = eng.lib, eng.h
    lens, alns, ops = np.zeros(64, np.uint32), np.zeros(ROOM, _lib.ALN_DT), np.zeros(ROOM, np.uint32)
    return {
        "get_read_lengths": ("reads", lambda: lib.bella_hip_get_read_lengths(h, lens.ctypes.data)),
        "get_dictionary": ("tuples", lambda: lib.bella_hip_get_dictionary(h, None, None)),
        "get_tuples": ("tuples", lambda: lib.bella_hip_get_tuples(h, None, None, None)),
        "panel_device_ptrs": ("panel", lambda: lib.bella_hip_panel_device_ptrs(h, None, None, None, None, None, None)),
        "get_B": ("matrix", lambda: lib.bella_hip_get_B(h, None, None, None, None)),
        "get_pairs": ("pairs", lambda: lib.bella_hip_get_pairs(h, None, None, None)),
        "get_alignments": ("alns", lambda: lib.bella_hip_get_alignments(h, alns.ctypes.data)),
        "get_traces": ("traces", lambda: lib.bella_hip_get_traces(h, None, None)),
        "get_batch_ops": ("batch_ops", lambda: lib.bella_hip_get_batch_ops(h, ops.ctypes.data, ROOM)),
    }


def _answers_as_the_model_says(eng, getters, first, valid, where):
    for name, (stage, get) in getters.items():
        rc = get()
        assert rc == (0 if stage in valid else STATE), (name, rc, where)
        if rc:
            assert eng.lib.bella_hip_last_error(eng.h).decode() == first[stage], (name, where)


def test_every_front_half_call_drops_what_the_table_says():
    import torch
    rs = synth.make_reads(**READS_40)
    eng = Engine(0)
    lib, h = eng.lib, eng.h
    pars = BellaPars(kmerSize=K)
    host = {}                                                         # what the later calls are fed with: tuples, B, seeds

    def count():
        host["nk"] = eng.count_kmers(K, LOWER, UPPER)[0]

    def fetch_tuples():
        host["t"] = eng.get_tuples()

    def fetch_B():
        host["B"] = eng.get_B()

    def overlap():
        assert 0 < eng.overlap(pars)[0] <= ROOM

    def trace_batch():
        pairs, a = eng.get_pairs()[0][:4], eng.get_alignments()[:4]
        seeds = np.zeros(4, _lib.SEED_DT)
        for f in seeds.dtype.names:
            seeds[f] = pairs[f]
        assert len(eng.trace_batch(seeds, a, pars)[1]) <= ROOM

    def panel_of(first, n):
        tk, tr, tp = host["t"]
        sel = (tr >= first) & (tr < first + n)
        return tk[sel], tr[sel], tp[sel]

    def set_B_refused():
        colptr = host["B"][0].copy()
        colptr[0] = 1
        return lib.bella_hip_set_B(h, K, host["nk"], colptr.ctypes.data, host["B"][1].ctypes.data, host["B"][2].ctypes.data)

    def set_B_device():
        colptr, rowids, values = (torch.as_tensor(a.astype(d)).cuda() for a, d in zip(host["B"], (np.int32, np.int32, np.int16)))
        eng.set_B_device(K, host["nk"], colptr, rowids, values)

    def too_large_a_k():
        tk, tr, tp = host["t"]
        return lib.bella_hip_assemble_tuples(h, 33, host["nk"], len(tk), tk.ctypes.data, tr.ctypes.data, tp.ctypes.data)

    def set_reads(v):
        made(v, "reads")
        changed(v, "records")

    def host_tuples(stage):                                           # the tuples come from the host: those of a count are overwritten
        def effect(v):
            for s in ("tuples", "panel", "matrix"):
                drop(v, s)
            if stage:
                made(v, stage)
        return effect

    def counted(stage):                                               # ... are on the device already: they stay
        def effect(v):
            for s in ("panel", "matrix"):
                drop(v, s)
            made(v, stage)
        return effect

    make = lambda stage: (lambda v: made(v, stage))
    change = lambda stage: (lambda v: changed(v, stage))
    nothing = lambda v: None
    to_traces = [("overlap", overlap, make("pairs")), ("align_pairs", lambda: eng.align_pairs(pars), make("alns")),
                 ("trace_pairs", lambda: eng.trace_pairs(pars), make("traces"))]
    script = [
        ("set_reads", lambda: eng.set_reads(rs), set_reads),
        ("count_kmers", count, make("tuples")),
        ("get_tuples", fetch_tuples, nothing),
        ("assemble_counted", eng.assemble_counted, counted("matrix")),
        ("get_B", fetch_B, nothing),
        *to_traces,
        ("graph_add_traced", eng.graph_add_traced, change("records")),
        ("graph_build", eng.graph_build, make("graph")),
        ("pileup_reset", eng.pileup_reset, make("pile")),
        ("trace_batch", trace_batch, make("batch_ops")),
        ("count_pairs", lambda: eng.count_pairs(pars), change("matrix")),       # drops the pairs and what follows them
        *to_traces,
        ("set_partition", lambda: eng.set_partition(1, 2), change("matrix")),   # drops the pairs, keeps the matrix
        *to_traces[:2],
        ("set_partition back", lambda: eng.set_partition(0, 1), change("matrix")),
        ("overlap", *to_traces[0][1:]),
        ("set_column_range", lambda: eng.set_column_range(0, 20), change("matrix")),
        ("overlap", *to_traces[0][1:]),
        ("set_column_range back", lambda: eng.set_column_range(0, 0xFFFFFFFF), change("matrix")),
        ("count_kmers again", count, make("tuples")),                           # a recount keeps the matrix
        *to_traces,
        ("assemble_tuples", lambda: eng.assemble_tuples(K, host["nk"], *host["t"]), host_tuples("matrix")),
        *to_traces,
        ("set_B refused past its drop point", set_B_refused, host_tuples(None), BAD_ARG),
        ("count_kmers", count, make("tuples")),
        ("assemble_panel", lambda: eng.assemble_panel(K, host["nk"], 0, 20, *panel_of(0, 20)), host_tuples("panel")),
        ("count_kmers", count, make("tuples")),                                 # ... keeps the panel too
        ("assemble_counted_panel", lambda: eng.assemble_counted_panel(20, 20), counted("panel")),
        ("set_B_panel", lambda: eng.set_B_panel(K, host["nk"], 0, 20, *host["B"]), host_tuples("panel")),
        ("count_kmers", count, make("tuples")),
        ("set_B_device", set_B_device, counted("matrix")),                      # keeps the tuples, drops the panel
        *to_traces,
        ("assemble_tuples refused before its drop point", too_large_a_k, nothing, BAD_ARG),
        ("assemble_counted_panel", lambda: eng.assemble_counted_panel(0, 20), counted("panel")),
        ("set_reads with a panel", lambda: eng.set_reads(rs), set_reads),       # the panel was one of the reads before
        ("count_kmers", count, make("tuples")),
        ("assemble_counted", eng.assemble_counted, counted("matrix")),
        *to_traces,
        ("set_reads with a matrix", lambda: eng.set_reads(rs), set_reads),
    ]
    getters, back = _front_getters(eng), _getters(eng)
    back["get_pileup"] = ("pile", lambda: lib.bella_hip_get_pileup(h, 0, 0, None))
    first = dict(FIRST, pile="bella_hip_pileup_reset first")
    valid = set()
    seen = set()
    _answers_as_the_model_says(eng, getters, FRONT_FIRST, valid, "in a new context")
    for step, (label, call, effect, *want) in enumerate(script):
        rc = call()
        assert (rc if isinstance(rc, int) and want else 0) == (want[0] if want else 0), (step, label, rc)
        effect(valid)
        where = "after step %d (%s), model %s" % (step, label, sorted(valid))
        _answers_as_the_model_says(eng, getters, FRONT_FIRST, valid, where)
        _answers_as_the_model_says(eng, back, first, valid, where)
        if label.startswith("set_reads"):
            n = C.c_uint64(99)
            assert lib.bella_hip_graph_get_overlaps(h, None, C.byref(n)) == 0 and n.value == 0, where
            assert not valid & set(first), where        # (the model itself: none of the back half's stages, which the getters above confirmed)
        seen.add(frozenset(valid & set(FRONT_FIRST)))
    assert len(seen) >= 8
    eng.close()


def test_allgather_panels_makes_the_matrix_and_drops_the_panel():
    rs = synth.make_reads(**READS_40)
    e0 = Engine(0)
    cid = e0.comm_id(local=True)
    engines = [Engine(0) for _ in range(2)]

    def body(r):
        e = engines[r]
        getters = _front_getters(e)
        valid = set()
        e.set_reads(rs)
        made(valid, "reads")
        e.comm_init(2, r, cid, local=True)
        e.count_kmers_dist(20 * r, 20, K, LOWER, UPPER)
        made(valid, "tuples")
        e.assemble_counted_panel(20 * r, 20)
        made(valid, "panel")
        _answers_as_the_model_says(e, getters, FRONT_FIRST, valid, "rank %d with its panel" % r)
        e.allgather_panels()
        drop(valid, "panel")
        made(valid, "matrix")
        _answers_as_the_model_says(e, getters, FRONT_FIRST, valid, "rank %d after the exchange" % r)
        return e.get_B()
    out, err = run_ranks(2, body, timeout=60)
    assert not err, err
    e0.set_reads(rs)
    e0.count_kmers(K, LOWER, UPPER)
    e0.assemble_counted()
    for B in out:
        assert all(np.array_equal(a, b) for a, b in zip(B, e0.get_B()))
    for e in engines:
        e.comm_destroy()
        e.close()
    e0.close()


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
