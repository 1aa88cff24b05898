"""CPU tests of the bubble-popping definition, on its mirror bella_testkit/bubble_mirror.py: the hand-stated
results of the inputs, detect's independence of the pop order, the mirror bubble, the graph after a pop, the ABI structs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bella_amd import _lib
from bella_testkit import bubble_mirror as B
from bella_testkit import graph_mirror as G
from bella_testkit import unitig_mirror as U
from conftest import ROOT


@pytest.fixture(scope="module")
def inputs():
    """name -> (lens, recs, pop parameters, the built graph, the popped one): computed once, never changed"""
    out = {}
    both = dict(B.named_inputs())
    both.update(B.existing_inputs())
    for name, (lens, recs, params) in both.items():
        m = G.build(recs, lens)
        out[name] = (lens, recs, params, m, B.pop(m["offsets"], m["edges"], m["contained"], None, **params))
    return out


def _unitigs(lens, m, r):
    u = U.unitigs(r["offsets"], r["edges"], m["contained"], r["removed"], lens)
    U.check_invariants(u, r["offsets"], r["edges"], m["contained"], r["removed"], lens)
    return u


def _ids(layout, variant="plain", **kw):
    return layout.build(variant, **kw)[2]


def test_simple(inputs):
    """the count decides, then the length, then the smaller predecessor"""
    for kind, gone in (("count", ["m14", "m15"]), ("length", ["m14", "m15"]), ("pred", ["x0", "x1"])):
        ids = _ids(B.simple_layout(kind))
        lens, _, _, m, r = inputs["simple-%s/plain" % kind]
        assert np.flatnonzero(r["removed"]).tolist() == sorted(ids[x] for x in gone), kind
        assert r["rounds"] == [(2, 1, 1, 2, 6), (0, 0, 0, 0, 0)]
        for var in B.VARIANTS:
            lens, _, _, m, r = inputs["simple-%s/%s" % (kind, var)]
            u = _unitigs(lens, m, r)
            assert r["rounds"] == [(2, 1, 1, 2, 6), (0, 0, 0, 0, 0)] and len(u["len"]) == 1 and not u["circular"][0] and len(u["verts"]) == 30 + (kind == "count")
    # 'pred': the kept predecessor of t is the smaller vertex, whatever the ids are
    lens, _, _, m, r = inputs["simple-pred/reversed"]
    ids = _ids(B.simple_layout("pred"), "reversed")
    assert np.flatnonzero(r["removed"]).tolist() == sorted(ids[x] for x in ("m14", "m15"))


def test_direct(inputs):
    for var in B.VARIANTS:
        lens, _, _, m, r = inputs["direct/" + var]
        assert r["rounds"] == [(2, 1, 1, 0, 2), (0, 0, 0, 0, 0)] and not r["removed"].any() and len(m["edges"]) - len(r["edges"]) == 2
        assert len(_unitigs(lens, m, r)["len"]) == 1
    off, e = B.literal_direct()                                       # s -> a -> t plus s -> t, which no build leaves
    r = B.pop(off, e, np.zeros(5, np.uint8), None)
    assert r["rounds"] == [(2, 1, 1, 0, 2), (0, 0, 0, 0, 0)] and not r["removed"].any()
    assert sorted(zip(r["edges"]["src"].tolist(), r["edges"]["dst"].tolist())) == sorted([(0, 2), (2, 4), (4, 6), (6, 8), (9, 7), (7, 5), (5, 3), (3, 1)])


def test_nested(inputs):
    """the inner source smaller: the inner bubble pops in round 1, the outer in round 2; the outer smaller: one round takes both"""
    two, one = [(4, 2, 1, 1, 4), (2, 1, 1, 1, 4), (0, 0, 0, 0, 0)], [(4, 2, 1, 2, 8), (0, 0, 0, 0, 0)]
    for name, var, want in (("nested-inner", "plain", two), ("nested-inner", "strands", two), ("nested-inner", "reversed", one),
                            ("nested-outer", "plain", one), ("nested-outer", "strands", one), ("nested-outer", "reversed", two)):
        lens, _, _, m, r = inputs["%s/%s" % (name, var)]
        u = _unitigs(lens, m, r)
        assert r["rounds"] == want and int(r["removed"].sum()) == 2 and len(u["len"]) == 1 and len(u["verts"]) == 9, (name, var)
    ids = _ids(B.nested_layout(), order=B.NESTED_OUTER_FIRST)
    assert ids["b"] in np.flatnonzero(inputs["nested-outer/plain"][4]["removed"]).tolist()       # s -> a -> c|d -> e -> t has more reads than s -> b -> t


def test_adjacent_and_shared_sink(inputs):
    for var in B.VARIANTS:
        lens, _, _, m, r = inputs["adjacent/" + var]
        assert r["rounds"] == [(4, 2, 2, 2, 8), (0, 0, 0, 0, 0)] and len(_unitigs(lens, m, r)["len"]) == 1
        lens, _, _, m, r = inputs["shared-sink/" + var]               # two forks into one vertex: neither is closed
        assert r["rounds"] == [(3, 0, 0, 0, 0)] and r["edges"].tobytes() == m["edges"].tobytes()


def test_refused(inputs):
    names = ["refused-%s/%s" % (k, v) for k in ("tip", "in", "out", "back", "dist", "reads1", "reads2", "reads255") for v in B.VARIANTS] + ["refused-both/plain"]
    for name in names:
        lens, _, _, m, r = inputs[name]
        assert len(r["rounds"]) == 1 and r["rounds"][0][0] >= 1 and r["rounds"][0][1:] == (0, 0, 0, 0), name
        assert r["edges"].tobytes() == m["edges"].tobytes() and np.array_equal(r["offsets"], m["offsets"]) and not r["removed"].any()
    for name, reads in (("popped-dist", 1), ("popped-reads3", 1), ("popped-reads255", 127)):
        for var in B.VARIANTS:
            lens, _, _, m, r = inputs["%s/%s" % (name, var)]
            assert r["rounds"][0][1:4] == (1, 1, reads) and len(_unitigs(lens, m, r)["len"]) == 1, name


def test_refusal_reasons():
    """in the definition's own order every refused graph fails for the reason it was made for"""
    def reasons(lens, recs, **params):
        m = G.build(recs, lens)
        o, e = [int(x) for x in m["offsets"]], (m["edges"]["dst"].tolist(), m["edges"]["len"].tolist())
        p = B._pop_params(params)
        why = []
        for s in range(len(o) - 1):
            if o[s + 1] - o[s] >= 2:
                assert B.detect(o, e, s, p, why=why) is None
        return set(why)
    for kind, params, want in (("tip", {}, "tip"), ("in", {}, "open"), ("back", {}, "cycle"), ("dist", dict(max_bubble_dist=5000), "dist"),
                               ("reads3", dict(max_bubble_reads=2), "reads"), ("reads256", dict(max_bubble_reads=255, max_bubble_dist=10 ** 6), "reads")):
        lens, recs, _, _ = B.refused_layout(kind).build()
        assert want in reasons(lens, recs, **params), kind
    assert "cycle" in reasons(*B.both_orientations())


@pytest.mark.parametrize("seed", range(20))
def test_chain(inputs, seed):
    """12 bubbles in a line: all pop in round 1 and ONE linear unitig is left, whose reads are the kept paths'"""
    lens, recs, _, m, r = inputs["chain-%d/strands" % seed]
    u = _unitigs(lens, m, r)
    assert r["rounds"][0][:3] == (24, 12, 12) and r["rounds"][1:] == [(0, 0, 0, 0, 0)]
    assert len(u["len"]) == 1 and not u["circular"][0] and len(u["links"]) == 0
    o, e = [int(x) for x in m["offsets"]], (m["edges"]["dst"].tolist(), m["edges"]["len"].tolist())
    p = B._pop_params({})
    kept = 0
    for s in range(len(o) - 1):
        b = B.detect(o, e, s, p) if o[s + 1] - o[s] >= 2 else None
        if b is not None and s < (b["t"] ^ 1):
            kept += len(B.kept_path(b, s)) - 1                        # the path's reads without s
    assert len(u["verts"]) == 3 + kept + 2                            # h0, h1, j0, the paths, z0, z1


def test_both_canonical_sides_occur(inputs):
    sides = set()
    for name, (_, _, _, _, r) in inputs.items():
        sides |= r["sides"]
    assert sides == {0, 1}


def test_existing_inputs_hold_no_bubble(inputs):
    for name in ("tip_input", "circle_input", "hub", "truth_chain"):
        r = inputs[name][4]
        print("BUBBLE", name, r["rounds"])
        assert len(r["rounds"]) == 1 and r["rounds"][0][1:] == (0, 0, 0, 0), name
    assert inputs["hub"][4]["rounds"][0][0] == 2999


def test_detect_does_not_depend_on_the_order(inputs):
    """20 random pop orders with shuffled edge visiting order: identical (t, visited, d, c, D, p) on every source; the mirror bubble
    (t ^ 1, s ^ 1) is found with the same reads"""
    rng = np.random.default_rng(99)
    nfound = 0
    for name, (lens, recs, params, m, _) in inputs.items():
        o, e = [int(x) for x in m["offsets"]], (m["edges"]["dst"].tolist(), m["edges"]["len"].tolist())
        p = B._pop_params(params)
        for s in range(len(o) - 1):
            if o[s + 1] - o[s] < 2:
                continue
            want = B.detect(o, e, s, p)
            for _ in range(20):
                assert B.detect(o, e, s, p, order=rng) == want, (name, s)
            if want is not None:
                nfound += 1
                t = want["t"]
                assert o[(t ^ 1) + 1] - o[t ^ 1] >= 2 and s != t ^ 1
                mir = B.detect(o, e, t ^ 1, p)
                assert mir is not None and mir["t"] == s ^ 1 and {x >> 1 for x in mir["visited"]} == {x >> 1 for x in want["visited"]}, (name, s)
    assert nfound > 500


def test_graph_after_a_pop(inputs):
    for name, (lens, recs, params, m, r) in inputs.items():
        B.check_graph(r["offsets"], r["edges"], r["removed"])
        _unitigs(lens, m, r)


def test_parameters():
    off, e = B.literal_direct()
    cont = np.zeros(5, np.uint8)
    assert B.pop(off, e, cont, None, max_bubble_reads=0)["rounds"] == [] and B.pop(off, e, cont, None, bubble_rounds=0)["rounds"] == []
    assert B.pop(off, e, cont, None, bubble_rounds=1)["rounds"] == [(2, 1, 1, 0, 2)]
    for bad in (dict(bubble_rounds=17), dict(max_bubble_reads=256)):
        with pytest.raises(ValueError):
            B.pop(off, e, cont, None, **bad)
    with pytest.raises(TypeError):
        B.pop(off, e, cont, None, max_tip_reads=1)


def test_bubble_structs_equal_the_header_as_a_c_compiler_sees_them(tmp_path):
    structs = {"bella_graph_bubble_params": _lib.GraphBubbleParams, "bella_bubble_stats": _lib.BubbleStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            src.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    src.append('printf("max reads %d\\n", BELLA_MAX_BUBBLE_READS); printf("max rounds %d\\n", BELLA_MAX_BUBBLE_ROUNDS);')
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert got[("max", "reads")] == _lib.MAX_BUBBLE_READS == B.MAX_BUBBLE_READS and got[("max", "rounds")] == _lib.MAX_BUBBLE_ROUNDS == B.MAX_BUBBLE_ROUNDS
    assert ctypes.sizeof(_lib.GraphBubbleParams) == 16


def test_cli_refuses_the_options_without_their_context():
    from bella_amd import build as b
    exe = b.build_cli()
    for flags, word in ((["--bubble-reads", "3"], "need --pop-bubbles"), (["--pop-bubbles"], "--pop-bubbles needs"), (["--pop-bubbles", "--gfa", "g", "--gfa-clean", "--bubble-reads", "256"], "[0, 255]"),
                        (["--pop-bubbles", "--unitigs", "u", "--bubble-rounds", "17"], "[0, 16]")):
        p = subprocess.run([exe, "-f", "none.txt", "-o", "none"] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and word in p.stderr.decode(), flags
