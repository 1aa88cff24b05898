"""GPU tests of bubble popping: through Engine, the device result EQUALS the mirror (bella_testkit/bubble_mirror.py)
-- popped CSR, removed flags, every per-round count, and the unitigs and bases that follow -- on every input of the CPU tests; state and
errors; the composition with graph_clean; bella-hip --pop-bubbles end to end on a diploid read set."""
import ctypes as C

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib, api
from bella_testkit import bubble_mirror as B
from bella_testkit import graph_mirror as G
from bella_testkit import synth
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import run_cli

pytestmark = pytest.mark.gpu

ARRAYS = ("voff", "verts", "pos", "nbases", "len", "circular", "links")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    both = dict(B.named_inputs())
    both.update(B.existing_inputs())
    return both


def _load(eng, lens, recs, seed=77):
    seqs = B.dummy_seqs(lens, seed)
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_add_overlaps(recs)
    return seqs


def _graph_is(eng, g, contained):
    off, e, cont = eng.graph()
    assert np.array_equal(off, g["offsets"]) and e.tobytes() == g["edges"].tobytes() and np.array_equal(cont, contained)
    assert np.array_equal(eng.graph_removed(), g["removed"])


def _stats_are(eng, r, edges_before):
    st = eng.bubble_stats()
    got = list(zip(st["sources"], st["found"], st["popped"], st["reads_per_round"], st["edges_per_round"]))
    assert got == r["rounds"] and st["rounds"] == len(r["rounds"]), (got, r["rounds"])
    assert st["reads_removed"] == sum(x[3] for x in r["rounds"]) and st["edges_removed"] == edges_before - len(r["edges"])
    return st


def _unitigs_are(eng, g, contained, lens, seqs):
    mu = U.unitigs(g["offsets"], g["edges"], contained, g["removed"], lens)
    du = eng.graph_unitigs()
    for k in ARRAYS:
        assert du[k].dtype == mu[k].dtype and du[k].tobytes() == mu[k].tobytes(), k
    moffs, mb = U.unitig_bases(mu, seqs)
    offs, bases = eng.unitig_bases()
    assert np.array_equal(offs, moffs) and bases.tobytes() == mb
    return mu


def _pop_equals_the_mirror(eng, lens, recs, params):
    seqs = _load(eng, lens, recs)
    m = G.build(recs, lens)
    eng.graph_build()
    r = B.pop(m["offsets"], m["edges"], m["contained"], None, **params)
    eng.graph_pop_bubbles(**params)
    _graph_is(eng, r, m["contained"])
    _stats_are(eng, r, len(m["edges"]))
    return r, _unitigs_are(eng, r, m["contained"], lens, seqs)


def test_every_named_input_equals_the_mirror(eng, inputs):
    """simple, direct, nested, adjacent, refused, chain, line, empty, one read, in their variants"""
    npopped = 0
    for name in B.named_inputs():
        lens, recs, params = inputs[name]
        r, mu = _pop_equals_the_mirror(eng, lens, recs, params)
        npopped += sum(x[2] for x in r["rounds"])
        if name.startswith("chain-"):
            assert len(mu["len"]) == 1 and r["rounds"][0][:3] == (24, 12, 12)
        if name.startswith("refused-"):
            assert r["rounds"][0][1:] == (0, 0, 0, 0)
    assert npopped > 250


@pytest.mark.parametrize("name", ["tip_input", "circle_input", "hub", "truth_chain"])
def test_the_graph_and_unitig_tests_inputs_equal_the_mirror(eng, inputs, name):
    lens, recs, params = inputs[name]
    r, _ = _pop_equals_the_mirror(eng, lens, recs, params)
    print("BUBBLE %s: rounds %s, %.3f ms" % (name, r["rounds"], eng.bubble_stats()["pop_ms"]))


def test_rounds_and_parameters(eng, inputs):
    """bubble_rounds 1 and 2 on the nested input stop where the mirror stops; max_bubble_reads 0 and bubble_rounds 0 do nothing"""
    lens, recs, _ = inputs["nested-inner/plain"]
    seqs = _load(eng, lens, recs)
    m = G.build(recs, lens)
    for params in (dict(bubble_rounds=1), dict(bubble_rounds=2), dict(max_bubble_reads=0), dict(bubble_rounds=0), dict(max_bubble_reads=4), dict(max_bubble_dist=3999)):
        eng.graph_build()
        r = B.pop(m["offsets"], m["edges"], m["contained"], None, **params)
        eng.graph_pop_bubbles(**params)
        _graph_is(eng, r, m["contained"])
        _stats_are(eng, r, len(m["edges"]))
        _unitigs_are(eng, r, m["contained"], lens, seqs)
    assert B.pop(m["offsets"], m["edges"], m["contained"], None, bubble_rounds=2)["rounds"] == [(4, 2, 1, 1, 4), (2, 1, 1, 1, 4)]


def _tips_and_bubbles():
    """a chain of bubbles with tips on it: two reads that hang off the side of an arm, and one off a junction.  (Six reads before and
    after the chain: a line end of up to max_tip_reads reads next to a fork is a tip itself.)"""
    y = B.chain_layout(3, nbubbles=6, ends=6)
    y.path(["b2_0_0", "tip0", "tip1"], 3000)
    y.link("j4", "tip2", 3500)
    return y.build("strands", seed=5)[:2]


def test_clean_and_pop_compose_as_the_mirrors_do(eng):
    lens, recs = _tips_and_bubbles()
    seqs = _load(eng, lens, recs)
    m = G.build(recs, lens)
    # clean, then pop (the driver's order)
    eng.graph_build()
    c = U.clean(m["offsets"], m["edges"], m["contained"])
    eng.graph_clean()
    r = B.pop(c["offsets"], c["edges"], m["contained"], c["removed"])
    eng.graph_pop_bubbles()
    _graph_is(eng, r, m["contained"])
    _stats_are(eng, r, len(c["edges"]))
    mu = _unitigs_are(eng, r, m["contained"], lens, seqs)
    assert c["removed"].sum() == 3 and sum(x[2] for x in r["rounds"]) == 6 and len(mu["len"]) == 1
    ust = eng.unitig_stats()                                          # the clean's figures stay
    assert list(zip(ust["tips_per_round"], ust["reads_per_round"])) == c["rounds"]
    # pop, then clean
    eng.graph_build()
    r2 = B.pop(m["offsets"], m["edges"], m["contained"], None)
    eng.graph_pop_bubbles()
    _graph_is(eng, r2, m["contained"])
    c2 = U.clean(r2["offsets"], r2["edges"], m["contained"])
    c2["removed"] = c2["removed"] | r2["removed"]
    eng.graph_clean()
    _graph_is(eng, c2, m["contained"])
    _stats_are(eng, r2, len(m["edges"]))                              # the pop's figures stay
    _unitigs_are(eng, c2, m["contained"], lens, seqs)
    assert sum(x[2] for x in r2["rounds"]) < 6                         # the tips keep some bubbles open until they are clipped


def test_state_and_errors(eng, inputs):
    lens, recs, _ = inputs["simple-count/plain"]
    seqs = _load(eng, lens, recs)
    for call in (eng.graph_pop_bubbles, eng.bubble_stats):            # no graph yet
        with pytest.raises(api.BellaHipError) as ex:
            call()
        assert ex.value.code == -7, call
    eng.graph_build()
    assert eng.bubble_stats()["rounds"] == 0 and eng.bubble_stats()["reads_removed"] == 0
    size = C.sizeof(_lib.GraphBubbleParams)
    for bad in (_lib.GraphBubbleParams(size - 4, 64, 50000, 3), _lib.GraphBubbleParams(size, 64, 50000, _lib.MAX_BUBBLE_ROUNDS + 1),
                _lib.GraphBubbleParams(size, _lib.MAX_BUBBLE_READS + 1, 50000, 3)):
        assert eng.lib.bella_hip_graph_pop_bubbles(eng.h, C.byref(bad)) == -3
    off0, e0, _ = eng.graph()
    eng.graph_unitigs()
    assert eng.lib.bella_hip_graph_pop_bubbles(eng.h, None) == 0       # NULL: the defaults
    m = G.build(recs, lens)
    r = B.pop(m["offsets"], m["edges"], m["contained"], None)
    _graph_is(eng, r, m["contained"])
    assert len(r["edges"]) < len(e0) and eng.bubble_stats()["rounds"] == 2
    with pytest.raises(api.BellaHipError) as ex:                     # a pop drops the unitigs
        eng.unitig_bases()
    assert ex.value.code == -7
    big = _lib.GraphBubbleParams(size + 8, 64, 50000, 3)               # a larger struct of a later header is read as far as this one goes
    assert eng.lib.bella_hip_graph_pop_bubbles(eng.h, C.byref(big)) == 0
    eng.graph_build()                                                 # a new build drops the stats and the removed reads
    assert eng.bubble_stats()["rounds"] == 0 and not eng.graph_removed().any()
    eng.graph_pop_bubbles()
    eng.graph_reset()                                                 # a reset, new records and other reads drop the graph and the stats with it
    with pytest.raises(api.BellaHipError) as ex:
        eng.bubble_stats()
    assert ex.value.code == -7
    eng.graph_add_overlaps(recs)
    eng.graph_build()
    eng.graph_pop_bubbles()
    eng.graph_add_overlaps(recs[:0])
    with pytest.raises(api.BellaHipError) as ex:
        eng.bubble_stats()
    assert ex.value.code == -7
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    for call in (eng.graph_pop_bubbles, eng.bubble_stats):
        with pytest.raises(api.BellaHipError) as ex:
            call()
        assert ex.value.code == -7
    with pytest.raises(TypeError):
        eng.graph_pop_bubbles(max_tip_reads=2)


# ---- command line ----------------------------------------------------------------------------------------------------------------
def _run(*args):
    files = run_cli(*args)
    return tuple(files.get(n) for n in ("g.gfa", "u.gfa", "u.fa")), files["stderr"].decode()      # (the log lines go to stderr)


def test_cli_pop_bubbles_end_to_end(eng, tmp_path):
    """A diploid read set: two copies of a random genome of 60 kb, a stretch of 3 kb replaced in one copy, exact reads of 8 kb every 1 kb
    from both.  (-u 40: every k-mer outside the stretch is in 16 reads, over the default upper bound of 8.)  bella-hip --unitigs
    --unitigs-fasta --gfa --gfa-clean --pop-bubbles writes what the Python path (trace -> records -> build -> clean -> pop -> unitigs) gives
    for the same input; without --pop-bubbles, what that path gives without the pop; -m 1 and -g 2 write the same files.  Whether the
    overlapper's graph of this set holds a bubble that pops is printed, not asserted (DESIGN.md section 13 records it: on an MI355X found
    [1, 0], popped [1, 0], 3 reads removed; 4 unitigs without the pop, 1 with it)."""
    glen, rl, step = 60000, 8000, 1000
    a = U.random_genome(glen, 61)
    b = a[:28000] + U.random_genome(3000, 62) + a[31000:]
    seqs = [hap[s:s + rl] for hap in (a, b) for s in range(0, glen - rl + 1, step)]
    strands = np.random.default_rng(63).integers(0, 2, len(seqs))
    seqs = [U.revcomp(s) if o else s for s, o in zip(seqs, strands)]
    rs = synth.ReadSet.from_strings(seqs)
    fq = str(tmp_path / "diploid.fastq")
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

    def python_path(pop):
        eng.graph_build()
        off, e, cont = eng.graph()
        eng.graph_clean()
        if pop:
            eng.graph_pop_bubbles()
        coff, ce, _ = eng.graph()
        dead = cont | eng.graph_removed()
        u = eng.graph_unitigs()
        offs, bases = eng.unitig_bases()
        return (G.gfa_text(names, lens, seqs, coff, ce, dead), U.unitig_gfa_text(names, u, offs, bases.tobytes()), U.fasta_text(u, offs, bases.tobytes())), len(u["len"])
    want_pop, n_pop = python_path(True)
    st = eng.bubble_stats()
    want_plain, n_plain = python_path(False)
    print("DIPLOID %d reads: bubbles found %s popped %s, reads removed %d; unitigs %d without, %d with the pop" % (len(seqs), st["found"], st["popped"], st["reads_removed"], n_plain, n_pop))
    flags = ["-u", "40", "--gfa", "g.gfa", "--gfa-clean", "--unitigs", "u.gfa", "--unitigs-fasta", "u.fa"]
    over = {"BELLA_HIP_OVERSUBSCRIBE": "1"}
    files, log = _run([fq], flags + ["--pop-bubbles"], str(tmp_path / "pop"))
    assert files == want_pop
    assert "%d bubbles popped, %d reads, " % (sum(st["popped"]), st["reads_removed"]) in log
    files, log = _run([fq], flags, str(tmp_path / "plain"))
    assert files == want_plain and "Unitigs = " in log and "bubbles popped" not in log
    assert _run([fq], flags + ["--pop-bubbles", "-m", "1"], str(tmp_path / "m1"))[0] == want_pop
    assert _run([fq], flags + ["--pop-bubbles", "-g", "2"], str(tmp_path / "g2"), over)[0] == want_pop
    files, _ = _run([fq], flags + ["--pop-bubbles", "--bubble-reads", "0"], str(tmp_path / "off"))
    assert files == want_plain
