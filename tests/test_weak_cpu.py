"""CPU tests of weak-overlap removal: the mirror (bella_testkit/weak_mirror.py) on every named input and against the
figures worked out by hand, the schedule of the command line, the new structs against the header, the command line's usage text and
argument errors.  The device is held to this mirror in test_weak_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bella_amd import _lib, api
from bella_testkit import bubble_mirror as B
from bella_testkit import graph_mirror as G
from bella_testkit import unitig_mirror as U
from bella_testkit import weak_mirror as W
from conftest import ROOT

RATIOS = (1, 300, 400, 500, 501, 700, 1000)


@pytest.fixture(scope="module")
def graphs():
    """name -> (lens, the mirror's graph of the input): built once, never changed"""
    return {name: (lens, G.build(recs, lens)) for name, (lens, recs) in W.named_inputs().items()}


def _cut(m, r):
    c = W.cut(m["offsets"], m["edges"], r)
    B.check_graph(c["offsets"], c["edges"], np.zeros((len(m["offsets"]) - 1) // 2, bool))      # twin-symmetric, CSR consistent
    return c


def test_every_named_input(graphs):
    """after every cut the graph is twin-symmetric and its CSR consistent; the surviving edges are the input's, byte for byte and in its
    order; the removed edges come in twin pairs, at least one of a pair weak; a rising ratio never cuts less; nothing is weak at a vertex
    with one out-edge; permille 0 and an edgeless graph give the input back"""
    assert {n.split("/")[0] for n in graphs} >= {"two-lines", "one-sided", "equal", "boundary", "line", "empty", "one-read", "tip_input", "circle_input", "hub", "truth_chain"}
    for name, (lens, m) in graphs.items():
        e0 = m["edges"]
        deg = np.diff(m["offsets"].astype(np.int64))
        before = -1
        for r in RATIOS:
            c = _cut(m, r)
            assert c["forks"] == (int((deg >= 2).sum()) if len(e0) else 0), name
            assert c["weak"] <= c["edges_removed"] <= 2 * c["weak"] and c["edges_removed"] % 2 == 0 and len(c["edges"]) == len(e0) - c["edges_removed"], (name, r)
            keys = (e0["src"].astype(np.int64) << 32) | e0["dst"]
            kept = np.isin(keys, (c["edges"]["src"].astype(np.int64) << 32) | c["edges"]["dst"])
            assert c["edges"].tobytes() == e0[kept].tobytes(), (name, r)
            gone = e0[~kept]
            assert not np.any(deg[gone["src"]] < 2) or c["weak"] < c["edges_removed"], (name, r)
            assert c["edges_removed"] >= before, (name, r)
            before = c["edges_removed"]
        z = W.cut(m["offsets"], m["edges"], 0)
        assert np.array_equal(z["offsets"], m["offsets"]) and z["edges"].tobytes() == e0.tobytes() and (z["forks"], z["weak"], z["edges_removed"]) == (0, 0, 0)
        if not len(e0):
            for r in RATIOS:
                c = W.cut(m["offsets"], e0, r)
                assert np.array_equal(c["offsets"], m["offsets"]) and len(c["edges"]) == 0 and (c["forks"], c["weak"], c["edges_removed"]) == (0, 0, 0)
    for name in ("line/plain", "circle_input", "truth_chain"):          # no fork, nothing to cut at any ratio
        assert _cut(graphs[name][1], 1000)["edges_removed"] == 0, name


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_two_lines(graphs, variant):
    """120 edges, 6 unitigs raw and still 6 after the default clean and pop; the cut at 500 takes the two false links with their twins and
    leaves the two lines, 68,000 bases each; 400 takes one link, 300 none"""
    lens, m = graphs["two-lines/" + variant]
    assert len(m["edges"]) == 120 and not m["contained"].any()
    assert len(U.unitigs(m["offsets"], m["edges"], m["contained"], None, lens)["len"]) == 6
    c = U.clean(m["offsets"], m["edges"], m["contained"])
    p = B.pop(c["offsets"], c["edges"], m["contained"], c["removed"])
    assert not p["removed"].any() and len(p["edges"]) == 120
    assert len(U.unitigs(p["offsets"], p["edges"], m["contained"], p["removed"], lens)["len"]) == 6
    k = _cut(p, 500)
    assert (k["forks"], k["weak"], k["edges_removed"]) == (4, 4, 4)
    u = U.unitigs(k["offsets"], k["edges"], m["contained"], p["removed"], lens)
    assert u["len"].tolist() == [68000, 68000] and len(u["links"]) == 0
    assert _cut(p, 400)["edges_removed"] == 2 and _cut(p, 300)["edges_removed"] == 0
    assert [_cut(p, r)["edges_removed"] for r in (375, 376, 437, 438)] == [0, 2, 2, 4]      # ovl 3,000 and 3,500 against 8,000: weak above 375 and above 437.5


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_one_sided_equal_and_boundary(graphs, variant):
    lens, m = graphs["one-sided/" + variant]
    for r in (376, 500, 1000):                                        # x -> m15 is x's only edge; its twin is weak at m15 ^ 1: both go
        c = _cut(m, r)
        assert (c["forks"], c["weak"], c["edges_removed"]) == (1, 1, 2)
    assert _cut(m, 375)["edges_removed"] == 0                          # 3,000,000 < 375 x 8,000 is false
    lens, m = graphs["equal/" + variant]
    for r in RATIOS:
        c = _cut(m, r)
        assert (c["forks"], c["weak"], c["edges_removed"]) == (1, 0, 0)
    lens, m = graphs["boundary/" + variant]
    assert (_cut(m, 500)["weak"], _cut(m, 500)["edges_removed"]) == (0, 0)      # 4,000,000 < 4,000,000 is false
    assert (_cut(m, 501)["weak"], _cut(m, 501)["edges_removed"]) == (1, 2)


def test_schedule(graphs):
    """the ratios; on two-lines with the spur the first cut leaves a tip of two reads that the clean behind it takes; without a cut
    nothing else runs"""
    assert W.ratios() == [500, 600, 700] and W.ratios(500, 700, 0) == [500] and W.ratios(1, 1000, 3) == [1, 334, 667, 1000] and W.ratios(400, 400, 16) == [400] * 17
    for bad in ((0, 700, 2), (701, 700, 2), (500, 1001, 2), (500, 700, 17), (500, 700, -1)):
        with pytest.raises(ValueError):
            W.ratios(*bad)
    assert W.SCHEDULE_DEFAULTS == dict(weak_min=500, weak_max=700, weak_steps=2) and W.WEAK_DEFAULTS == dict(api.Engine.WEAK_DEFAULTS) == dict(ratio_permille=500)
    for variant in B.VARIANTS:
        lens, m = graphs["two-lines-spur/" + variant]
        c = U.clean(m["offsets"], m["edges"], m["contained"])
        p = B.pop(c["offsets"], c["edges"], m["contained"], c["removed"])
        assert not p["removed"].any() and len(p["edges"]) == 126         # the spur is closed at both ends: no tip, no bubble
        for bubbles in (None, {}):
            s = W.schedule(p["offsets"], p["edges"], m["contained"], p["removed"], lens, clean_params={}, bubble_params=bubbles)
            got = [(x["ratio_permille"], x["edges_removed"], x["reads_clipped"], x["bubbles_popped"], x["unitigs"]) for x in s["steps"]]
            assert got == [(500, 6, 2, 0, 2), (600, 0, 0, 0, 2), (700, 0, 0, 0, 2)]
            assert s["removed"].sum() == 2 and len(s["edges"]) == 116
            B.check_graph(s["offsets"], s["edges"], s["removed"])
            assert U.unitigs(s["offsets"], s["edges"], m["contained"], s["removed"], lens)["len"].tolist() == [68000, 68000]
        s = W.schedule(p["offsets"], p["edges"], m["contained"], p["removed"], lens, 1, 300, 1, {}, {})
        assert [x["edges_removed"] for x in s["steps"]] == [0, 0] and s["edges"].tobytes() == p["edges"].tobytes() and not s["removed"].any()
    with pytest.raises(ValueError):
        W.cut(np.zeros(3, np.uint64), np.zeros(0, G.EDGE_DT), 1001)


def test_weak_structs_equal_the_header_as_a_c_compiler_sees_them(tmp_path):
    structs = {"bella_graph_weak_params": _lib.GraphWeakParams, "bella_weak_stats": _lib.WeakStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            src.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    for cname in ("bella_graph_bubble_params", "bella_bubble_stats", "bella_unitig_stats", "bella_graph_edge"):
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
    src.append('printf("abi version %d\\n", BELLA_HIP_ABI_VERSION);')
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    protos = tmp_path / "protos.c"                                    # the prototypes, as a C compiler reads them (compiled, not linked)
    protos.write_text('#include "bella_hip.h"\n'
                      'int (*cut)(bella_ctx*, const bella_graph_weak_params*) = bella_hip_graph_cut_weak;\n'
                      'int (*get)(bella_ctx*, void*, uint64_t) = bella_hip_graph_get_weak_stats;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(_lib.GraphWeakParams) == 8 and ctypes.sizeof(_lib.WeakStats) == 40
    # additive: the version and the neighbouring structs stay what they were
    assert got[("abi", "version")] == 6 and _lib.load().bella_hip_abi_version() == 6
    assert got[("bella_graph_bubble_params", "size")] == ctypes.sizeof(_lib.GraphBubbleParams) == 16 and got[("bella_bubble_stats", "size")] == ctypes.sizeof(_lib.BubbleStats)
    assert got[("bella_unitig_stats", "size")] == ctypes.sizeof(_lib.UnitigStats) and got[("bella_graph_edge", "size")] == 24


def _cli():
    from bella_amd import build as b
    return b.build_cli()


def test_cli_help_lists_the_options():
    p = subprocess.run([_cli(), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    text = p.stdout.decode()
    assert p.returncode == 0
    for opt in ("--cut-weak ", "--weak-min arg", "--weak-max arg", "--weak-steps arg"):
        assert opt in text, opt


def test_cli_refuses_the_options_without_their_context():
    """all of these are decided before a device is looked for"""
    need = "need --cut-weak"
    rng = "--weak-min and --weak-max must be in [1, 1000]"
    for flags, word in ((["--weak-min", "400", "--unitigs", "u"], need), (["--weak-max", "800", "--unitigs", "u"], need), (["--weak-steps", "1", "--gfa", "g", "--gfa-clean"], need),
                        (["--cut-weak"], "--cut-weak needs --unitigs, --unitigs-fasta or --gfa-clean"), (["--cut-weak", "--gfa", "g"], "--cut-weak needs --unitigs"),
                        (["--cut-weak", "--unitigs", "u", "--weak-min", "0"], rng), (["--cut-weak", "--unitigs", "u", "--weak-min", "701"], rng),
                        (["--cut-weak", "--unitigs-fasta", "u", "--weak-max", "1001"], rng), (["--cut-weak", "--gfa", "g", "--gfa-clean", "--weak-steps", "17"], rng),
                        (["--cut-weak", "--unitigs", "u", "--weak-steps", "-1"], rng), (["--cut-weak", "--unitigs", "u", "--skip-alignment"], "--skip-alignment")):
        p = subprocess.run([_cli(), "-f", "none.txt", "-o", "none"] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and word in p.stderr.decode(), (flags, p.stderr)
