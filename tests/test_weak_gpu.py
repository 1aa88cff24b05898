"""GPU tests of weak-overlap removal: through Engine, the device result EQUALS the mirror (bella_testkit/weak_mirror.py)
-- the cut CSR, the untouched flags, the counts, and the unitigs and bases that follow -- on every input of the CPU tests; parameters; state
and errors; the composition with graph_trim and with graph_clean / graph_pop_bubbles in the command line's schedule; bella-hip --cut-weak end
to end on a read set with a repeat."""
import ctypes as C

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib
from bella_testkit import bubble_mirror as B
from bella_testkit import graph_mirror as G
from bella_testkit import synth
from bella_testkit import trim_mirror as T
from bella_testkit import unitig_mirror as U
from bella_testkit import weak_mirror as W
from bella_testkit.pipeline import raises, run_cli

pytestmark = pytest.mark.gpu

ARRAYS = ("voff", "verts", "pos", "nbases", "len", "circular", "links")
STATE, BAD = -7, -3


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    """name -> (lens, recs, the mirror's graph): built once, never changed"""
    return {name: (lens, recs, G.build(recs, lens)) for name, (lens, recs) in W.named_inputs().items()}


def _load(eng, lens, recs, seed=77):
    seqs = B.dummy_seqs(lens, seed)
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_add_overlaps(recs)
    return seqs


def _graph_is(eng, g, contained, removed=None):
    off, e, cont = eng.graph()
    assert np.array_equal(off, g["offsets"]) and e.tobytes() == g["edges"].tobytes() and np.array_equal(cont, contained)
    assert np.array_equal(eng.graph_removed(), removed if removed is not None else np.zeros(len(contained), np.uint8))


def _stats_are(eng, c, r):
    st = eng.weak_stats()
    assert (st["forks"], st["weak"], st["edges_removed"], st["ratio_permille"]) == (c["forks"], c["weak"], c["edges_removed"], r), (st, r)
    return st


def _unitigs_are(eng, g, contained, removed, lens, seqs):
    mu = U.unitigs(g["offsets"], g["edges"], contained, removed, lens)
    du = eng.graph_unitigs()
    for k in ARRAYS:
        assert du[k].dtype == mu[k].dtype and du[k].tobytes() == mu[k].tobytes(), k
    moffs, mb = U.unitig_bases(mu, seqs)
    offs, bases = eng.unitig_bases()
    assert np.array_equal(offs, moffs) and bases.tobytes() == mb
    return mu


def _cut_equals_the_mirror(eng, m, lens, seqs, r):
    """after a graph_build of m's input: cut at r on the device and in the mirror"""
    c = W.cut(m["offsets"], m["edges"], r)
    eng.graph_cut_weak(ratio_permille=r)
    _graph_is(eng, c, m["contained"])
    st = _stats_are(eng, c, r)
    return c, _unitigs_are(eng, c, m["contained"], None, lens, seqs), st


def test_every_named_input_equals_the_mirror(eng, inputs):
    """two-lines, one-sided, equal, boundary, line in their variants; empty, one read; at the default ratio, and at 1000 where there is a fork"""
    ncut = 0
    for name, (lens, recs, m) in inputs.items():
        if "/" not in name:
            continue
        seqs = _load(eng, lens, recs)
        for r in (500, 1000):
            eng.graph_build()
            c, mu, _ = _cut_equals_the_mirror(eng, m, lens, seqs, r)
            ncut += c["edges_removed"]
            if name.startswith("two-lines/"):
                assert (c["forks"], c["weak"], c["edges_removed"]) == (4, 4, 4) and mu["len"].tolist() == [68000, 68000]
            if name.startswith("one-sided/"):
                assert (c["weak"], c["edges_removed"]) == (1, 2)
            if name.startswith("equal/"):
                assert (c["forks"], c["weak"], c["edges_removed"]) == (1, 0, 0)
    assert ncut > 60


@pytest.mark.parametrize("name", ["tip_input", "circle_input", "hub", "truth_chain"])
def test_the_graph_and_unitig_tests_inputs_equal_the_mirror(eng, inputs, name):
    """the hub is the input with long twin scans: 700 edges enter read 0 before the reduction"""
    lens, recs, m = inputs[name]
    seqs = _load(eng, lens, recs)
    for r in ((500, 700, 1000) if name == "hub" else (500, 1000)):
        eng.graph_build()
        c, _, st = _cut_equals_the_mirror(eng, m, lens, seqs, r)
        print("WEAK %s at %d: %d edges, max degree %d, forks %d, weak %d, removed %d, %.3f ms" % (name, r, len(m["edges"]), int(np.diff(m["offsets"].astype(np.int64)).max()),
                                                                                                 c["forks"], c["weak"], c["edges_removed"], st["cut_ms"]))


def test_parameters(eng, inputs):
    lens, recs, m = inputs["two-lines/strands"]
    seqs = _load(eng, lens, recs)
    want = {300: 0, 400: 2, 500: 4, 1000: 4}
    for r, n in want.items():
        eng.graph_build()
        c, _, _ = _cut_equals_the_mirror(eng, m, lens, seqs, r)
        assert c["edges_removed"] == n
    eng.graph_build()                                                 # 0 is off: nothing changes, the figures stay zero
    eng.graph_cut_weak(ratio_permille=0)
    _graph_is(eng, m, m["contained"])
    st = eng.weak_stats()
    assert (st["forks"], st["weak"], st["edges_removed"], st["ratio_permille"], st["cut_ms"]) == (0, 0, 0, 0, 0.0)
    size = C.sizeof(_lib.GraphWeakParams)
    assert size == 8
    assert eng.lib.bella_hip_graph_cut_weak(eng.h, C.byref(_lib.GraphWeakParams(size, 1001))) == BAD
    assert eng.lib.bella_hip_graph_cut_weak(eng.h, C.byref(_lib.GraphWeakParams(size - 4, 500))) == BAD
    _graph_is(eng, m, m["contained"])                                 # a refused call leaves the graph alone
    with pytest.raises(TypeError):
        eng.graph_cut_weak(max_tip_reads=2)
    assert eng.lib.bella_hip_graph_cut_weak(eng.h, None) == 0          # NULL: the defaults
    c = W.cut(m["offsets"], m["edges"])
    _graph_is(eng, c, m["contained"])
    _stats_are(eng, c, 500)

    class Later(C.Structure):                                         # a larger struct of a later header is read as far as this one goes
        _fields_ = [("struct_size", C.c_uint32), ("ratio_permille", C.c_uint32), ("more", C.c_uint32 * 2)]
    eng.graph_build()
    assert eng.lib.bella_hip_graph_cut_weak(eng.h, C.cast(C.byref(Later(size + 8, 400, (1001, 1001))), C.POINTER(_lib.GraphWeakParams))) == 0
    c = W.cut(m["offsets"], m["edges"], 400)
    _graph_is(eng, c, m["contained"])
    _stats_are(eng, c, 400)
    for var in B.VARIANTS:
        lens, recs, m = inputs["boundary/" + var]
        seqs = _load(eng, lens, recs)
        for r, n in ((500, 0), (501, 2)):
            eng.graph_build()
            c, _, _ = _cut_equals_the_mirror(eng, m, lens, seqs, r)
            assert c["edges_removed"] == n


def test_state_and_errors(eng, inputs):
    lens, recs, m = inputs["two-lines/plain"]
    seqs = _load(eng, lens, recs)
    for call in (eng.graph_cut_weak, eng.weak_stats):                 # no graph yet
        raises(STATE, call)
    eng.graph_trim(min_depth=1, end_clip=0)
    clips = eng.graph_clips()
    mc = T.clips(recs, lens, min_depth=1, end_clip=0)
    assert clips.tobytes() == mc.tobytes()
    mt = T.build(recs, lens, mc)
    eng.graph_build()
    zero = dict(forks=0, weak=0, edges_removed=0, ratio_permille=0, cut_ms=0.0)
    assert eng.weak_stats() == zero
    eng.graph_unitigs()
    eng.graph_cut_weak()
    c = W.cut(mt["offsets"], mt["edges"])
    _graph_is(eng, c, mt["contained"])
    assert c["edges_removed"] == 4 and _stats_are(eng, c, 500)["cut_ms"] > 0
    raises(STATE, eng.unitig_bases)                                   # a cut drops the unitigs
    assert eng.graph_clips().tobytes() == clips.tobytes()             # ... and keeps the trim
    eng.graph_build()                                                 # a new build zeroes the stats
    assert eng.weak_stats() == zero
    eng.graph_cut_weak()
    eng.graph_reset()                                                 # a reset, new records and other reads drop the graph and the stats with it
    raises(STATE, eng.weak_stats)
    eng.graph_add_overlaps(recs)
    eng.graph_build()
    eng.graph_cut_weak()
    eng.graph_add_overlaps(recs[:0])
    raises(STATE, eng.weak_stats)
    eng.graph_build()
    eng.graph_cut_weak()
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    for call in (eng.graph_cut_weak, eng.weak_stats):
        raises(STATE, call)


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_cut_of_a_trimmed_graph(eng, inputs, variant):
    """two-lines with junk at 30 % of the read ends; the trim clips it off, the build cuts the records to the clips, and the cut compares
    the overlaps in clipped coordinates: what it removes is what it removes without the junk (the reads at the lines' ends aside, which the
    trim shortens)"""
    lens, recs, _ = inputs["two-lines/" + variant]
    jl, jr, head, tail = T.junk_ends(None, lens, None, recs, 0.3, 1200, 3000)
    G.check_records(jr, jl)
    eng.set_reads(synth.ReadSet.from_strings(B.dummy_seqs(jl)))
    eng.graph_add_overlaps(jr)
    tp = dict(min_depth=1, end_clip=0, min_span=1000)
    eng.graph_trim(**tp)
    mc = T.clips(jr, jl, **tp)
    assert eng.graph_clips().tobytes() == mc.tobytes() and (mc["end"] - mc["beg"] < jl).sum() > 20
    m = T.build(jr, jl, mc)
    seqs = T.clip_seqs(B.dummy_seqs(jl), mc)
    for r in (400, 500):
        eng.graph_build()
        c = W.cut(m["offsets"], m["edges"], r)
        eng.graph_cut_weak(ratio_permille=r)
        _graph_is(eng, c, m["contained"])
        _stats_are(eng, c, r)
        _unitigs_are(eng, c, (m["contained"] != 0).astype(np.uint8), None, m["lens"], seqs)
        assert c["edges_removed"] == (2 if r == 400 else 4)
    plain = G.build(jr, jl)                                           # without the trim the junk changes the lengths the ratio is taken of
    assert W.cut(plain["offsets"], plain["edges"], 500)["edges"].tobytes() != c["edges"].tobytes()


def _engine_schedule(eng, weak_min=500, weak_max=700, weak_steps=2, clean=None, bubbles=None, after=None):
    """the command line's schedule as Engine calls: -> the steps' figures, as weak_mirror.schedule names them; after(i) runs behind step i"""
    steps = []
    for r in W.ratios(weak_min, weak_max, weak_steps):
        eng.graph_cut_weak(ratio_permille=r)
        st = eng.weak_stats()
        step = dict(ratio_permille=st["ratio_permille"], forks=st["forks"], weak=st["weak"], edges_removed=st["edges_removed"], reads_clipped=0, bubbles_popped=0)
        if st["edges_removed"]:
            eng.graph_clean(**(clean or {}))
            step["reads_clipped"] = eng.unitig_stats()["reads_removed"]
            if bubbles is not None:
                eng.graph_pop_bubbles(**bubbles)
                step["bubbles_popped"] = sum(eng.bubble_stats()["popped"])
        steps.append(step)
        if after:
            after(len(steps) - 1)
    return steps


FIGURES = ("ratio_permille", "forks", "weak", "edges_removed", "reads_clipped", "bubbles_popped")


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_the_schedule_composes_as_the_mirrors_do(eng, inputs, variant):
    """two-lines with the two-read spur: clean, pop, then the schedule; graph, removed flags and unitigs after every step"""
    lens, recs, m = inputs["two-lines-spur/" + variant]
    seqs = _load(eng, lens, recs)
    for bubbles in ({}, None):
        eng.graph_build()
        c = U.clean(m["offsets"], m["edges"], m["contained"])
        eng.graph_clean()
        p = c
        if bubbles is not None:
            p = B.pop(c["offsets"], c["edges"], m["contained"], c["removed"])
            eng.graph_pop_bubbles()
        _graph_is(eng, p, m["contained"], p["removed"])
        s = W.schedule(p["offsets"], p["edges"], m["contained"], p["removed"], lens, clean_params={}, bubble_params=bubbles)

        def after(i):
            x = s["steps"][i]
            _graph_is(eng, x, m["contained"], x["removed"])
            assert len(_unitigs_are(eng, x, m["contained"], x["removed"], lens, seqs)["len"]) == x["unitigs"]
        got = _engine_schedule(eng, clean={}, bubbles=bubbles, after=after)
        assert got == [{k: x[k] for k in FIGURES} for x in s["steps"]]
        assert [(x["edges_removed"], x["reads_clipped"]) for x in got] == [(6, 2), (0, 0), (0, 0)] and s["steps"][-1]["unitigs"] == 2
        _graph_is(eng, s, m["contained"], s["removed"])


# ---- command line ----------------------------------------------------------------------------------------------------------------
def _run(*args):
    files = run_cli(*args)
    return tuple(files.get(n) for n in ("g.gfa", "u.gfa", "u.fa")), files["stderr"].decode()      # (the log lines go to stderr)


def test_cli_cut_weak_end_to_end(eng, tmp_path):
    """Two random sequences of 40 kb that share one stretch of 3 kb at different places (a repeat with a copy in either), exact reads of 8 kb
    every 1 kb from both, random strands (-u 40 as in the diploid test).  bella-hip --gfa --gfa-clean --unitigs --unitigs-fasta --pop-bubbles
    --cut-weak writes what the Python path (trace -> records -> build -> clean -> pop -> the schedule as Engine calls -> unitigs) gives, and
    logs its sums; without --cut-weak, what that path gives without the schedule, and no WeakOverlaps line; -m 1 and -g 2 write the same
    files; --weak-steps 0 --weak-min 1 differs as the Python path says.  Whether this set's graph holds a weak edge, and the unitig counts
    with and without the option, are printed, not asserted (DESIGN.md section 17 records what an MI355X printed: 2 forks and no weak edge at
    500, 600 and 700 permille, 5 unitigs, the largest of 31,000 bases, with and without the option)."""
    glen, rl, step = 40000, 8000, 1000
    rep = U.random_genome(3000, 73)
    a, b = U.random_genome(glen, 71), U.random_genome(glen, 72)
    a = a[:12000] + rep + a[15000:]
    b = b[:26000] + rep + b[29000:]
    seqs = [g[s:s + rl] for g in (a, b) for s in range(0, glen - rl + 1, step)]
    strands = np.random.default_rng(74).integers(0, 2, len(seqs))
    seqs = [U.revcomp(s) if o else s for s, o in zip(seqs, strands)]
    rs = synth.ReadSet.from_strings(seqs)
    fq = str(tmp_path / "repeat.fastq")
    synth.write_fastq(fq, rs)
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 40)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    eng.align_pairs(pars)
    eng.trace_pairs_records(pars)
    eng.graph_reset()
    eng.graph_add_traced()
    lens, names = rs.lengths, rs.names

    def python_path(sched):
        eng.graph_build()
        off, e, cont = eng.graph()
        eng.graph_clean()
        eng.graph_pop_bubbles()
        steps = _engine_schedule(eng, clean={}, bubbles={}, **sched) if sched is not None else []
        coff, ce, _ = eng.graph()
        dead = cont | eng.graph_removed()
        u = eng.graph_unitigs()
        offs, bases = eng.unitig_bases()
        return (G.gfa_text(names, lens, seqs, coff, ce, dead), U.unitig_gfa_text(names, u, offs, bases.tobytes()), U.fasta_text(u, offs, bases.tobytes())), steps, u

    def log_line(steps):
        return "WeakOverlaps = %d edges cut in %d rounds at %d..%d permille, %d reads clipped after, %d bubbles popped after" % (
            sum(x["edges_removed"] for x in steps), len(steps), steps[0]["ratio_permille"], steps[-1]["ratio_permille"], sum(x["reads_clipped"] for x in steps),
            sum(x["bubbles_popped"] for x in steps))
    want_cut, steps, u_cut = python_path({})
    want_one, steps_one, _ = python_path(dict(weak_min=1, weak_steps=0))
    want_plain, _, u_plain = python_path(None)
    print("REPEAT %d reads: per step (permille, forks, weak, edges cut, reads clipped after, bubbles popped after) %s; unitigs %d (largest %d) without, %d (largest %d) with --cut-weak"
          % (len(seqs), [tuple(x[k] for k in FIGURES) for x in steps], len(u_plain["len"]), int(u_plain["len"].max()), len(u_cut["len"]), int(u_cut["len"].max())))
    flags = ["-u", "40", "--gfa", "g.gfa", "--gfa-clean", "--unitigs", "u.gfa", "--unitigs-fasta", "u.fa", "--pop-bubbles"]
    over = {"BELLA_HIP_OVERSUBSCRIBE": "1"}
    files, log = _run([fq], flags + ["--cut-weak"], str(tmp_path / "cut"))
    assert files == want_cut and log_line(steps) in log and [x["ratio_permille"] for x in steps] == [500, 600, 700]
    files, log = _run([fq], flags, str(tmp_path / "plain"))
    assert files == want_plain and "Unitigs = " in log and "WeakOverlaps" not in log
    assert _run([fq], flags + ["--cut-weak", "-m", "1"], str(tmp_path / "m1"))[0] == want_cut
    assert _run([fq], flags + ["--cut-weak", "-g", "2"], str(tmp_path / "g2"), over)[0] == want_cut
    files, log = _run([fq], flags + ["--cut-weak", "--weak-steps", "0", "--weak-min", "1"], str(tmp_path / "one"))
    assert files == want_one and log_line(steps_one) in log and " in 1 rounds at 1..1 permille" in log
