"""CPU tests of the circular realignment round: the unrolled-circle placement by hand, the error-free circle of
realign_cases.py polished with a gentle table (how many reads vote, how many reach across an origin, the fallback, the depth around the
origin and the distance to the true circle), the case list of the GPU tests, a noisy circle built from truth, the stats struct and
the new entry points against the header, and the command line's argument errors.  The device is held to this mirror in
test_realign_circular_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bella_amd import _lib
from bella_testkit import pileup_mirror as P
from bella_testkit import realign_cases as RC
from bella_testkit import realign_circle_cases as CC
from bella_testkit import realign_mirror as R
from bella_testkit import trim_mirror as TM
from bella_testkit import unitig_mirror as U
from conftest import ROOT


def test_the_unrolled_placement_by_hand():
    """three segments, raw length 300, current length 295 (test_realign_cpu.py's map); band_max 64, so the shift is below 32"""
    seg = (np.array([0, 100, 250]), np.array([100, 150, 50]), np.array([0, 90, 240]), np.array([90, 150, 55]))
    f = lambda x, n, bm=64: R.place_unrolled(x, n, *seg, 300, 295, bm)
    assert f(-20, 50) == (273, 322)                # x < 0 wraps to 280: s0 = 240 + 30 * 55 // 50; ym = 330: e0 = 295 + P(30) = 295 + 27
    assert f(280, 50) == f(-20, 50) == f(580, 50)
    assert f(260, 60) == (251, 313)                # the last segment, ym = 320 >= len: e0 = 295 + P(20) = 295 + 18
    assert f(250, 50) == (240, 295)                # ym == len: e0 = plen + P(0)
    assert f(10, 50) == (9 + 295, 54 + 295)        # s0 = 9 < 32: both ends move on by plen; e0 = P(60) = 54
    assert f(40, 50) == (36, 81)                   # s0 = 36 >= 32: no shift
    assert f(0, 600) is None                       # ym - len >= len
    assert f(0, 232) is None and f(0, 231) == (295, 295 + 221)      # max(n, e0 - s0) + band_max <= plen: 231 + 64 = 295; P(231) = 90 + 131
    assert f(0, 100, 256) is None                  # the same rule through band_max
    big = 1 << 29
    one = (np.array([0]), np.array([big]), np.array([0]), np.array([big]))
    assert R.place_unrolled(5, 100, *one, big, big, 64) is None                            # plen >= 2^29
    assert R.place_unrolled(5, 100, np.array([0]), np.array([big - 1]), np.array([0]), np.array([big - 1]), big - 1, big - 1, 64) == (5 + big - 1, 105 + big - 1)
    # a window that runs backwards (e0 < s0) cannot come from a monotone map; the rule still names it
    back = (np.array([0, 100]), np.array([100, 100]), np.array([50, 0]), np.array([50, 50]))
    assert R.place_unrolled(10, 100, *back, 200, 300, 64) is None


@pytest.fixture(scope="module")
def circle():
    """circle_case() polished with gentle_table(seed 3), and the rounds at band0 256 the tests below share"""
    seqs, recs = RC.circle_case()
    m, c, u = U.case_unitigs(seqs, recs, RC.GRAPH, {})
    assert u["circular"].tolist() == [1] and u["len"].tolist() == [6000]
    p = U.polished(u, seqs, CC.gentle_table(seqs, 3), 3)
    run = lambda **kw: R.realign_round(u, p, seqs, recs, m["contained"], c["removed"], None, band0=256, **kw)
    genome, strands = CC.circle_truth()
    truth = CC.unitig_template(genome, u, np.arange(12) * 500, np.full(12, 1500), strands)
    return dict(seqs=seqs, recs=recs, m=m, c=c, u=u, p=p, run=run, truth=truth, plain=run(band_max=4096), circ=run(band_max=4096, circular=True))


def _low(res, md=3):
    t = res["table"].astype(np.int64)
    return int(((t[:, 0:4].sum(1) + t[:, P.DEL]) < md).sum())


def test_every_read_of_the_circle_votes(circle):
    plen = len(circle["p"]["bases"])
    assert plen != 6000
    pl, cnt = circle["circ"]["placements"], circle["circ"]["counts"]
    assert (pl["status"] == R.VOTED).sum() == 12 and cnt["outside"] == 0 and cnt["voted"] == 12 and (pl["pad"] == 1).all()
    assert (circle["plain"]["placements"]["status"] == R.OUTSIDE).sum() == 2 and "wrapped" not in circle["plain"]["counts"]
    assert (circle["plain"]["placements"]["pad"] == 0).all()
    assert int((pl["e"] > plen).sum()) == 7 and cnt["wrapped"] >= 7
    assert (pl["s"] >= 2048).all() and (pl["s"] < plen + 2048).all()
    args = (circle["u"], circle["p"], [len(s) for s in circle["seqs"]], circle["recs"], circle["m"]["contained"], circle["c"]["removed"], None, 256)
    narrow, _ = R.place(*args, band_max=512, circular=True)
    assert int((narrow["e"] > plen).sum()) == 3 and (narrow["pad"] == 1).all()
    low = (_low(circle["circ"]), _low(circle["plain"]))
    print("REALIGN circle: %d bases polished; positions below depth 3: %d with the circle rule, %d without; wrapped %d" % (plen, low[0], low[1], cnt["wrapped"]))
    assert low[0] <= 16


def test_a_circle_shorter_than_read_plus_band_max_falls_back(circle):
    a, b = circle["run"](band_max=8192, circular=True), circle["run"](band_max=8192)
    assert a["counts"].pop("wrapped") == 0 and a["counts"] == b["counts"]
    for f in R.PLACE_DT.names:
        assert np.array_equal(a["placements"][f], b["placements"][f]), f
    assert np.array_equal(a["table"], b["table"]) and a["bases"] == b["bases"] and np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["nbases"], b["nbases"])
    assert (a["placements"]["status"] == R.OUTSIDE).sum() == 2


def test_the_circle_rule_brings_the_circle_closer_to_the_truth(circle):
    """Levenshtein distance of the whole unitig to the true circle, rotated to the unitig's first base: with the rule BELOW the plain
    round BELOW the polish.  Prototype: 3, 119, 330."""
    d = [P.edit_distance(bytes(x["bases"]), circle["truth"]) for x in (circle["circ"], circle["plain"], circle["p"])]
    print("REALIGN circle: edit distance to the true circle: circular %d, plain %d, polished %d" % tuple(d))
    assert d[0] < d[1] < d[2], d


def test_circle_plus_covers_what_the_gpu_tests_need():
    seqs, recs = CC.circle_plus()
    m, c, u = U.case_unitigs(seqs, recs, RC.GRAPH, {})
    assert u["circular"].tolist() == [1] and u["len"].tolist() == [6000] and m["contained"].tolist() == [0] * 12 + [1, 1]
    p = U.polished(u, seqs, CC.gentle_table(seqs, 3), 3)
    plen = len(p["bases"])
    r = R.realign_round(u, p, seqs, recs, m["contained"], c["removed"], None, band0=256, circular=True)
    pl = r["placements"]
    voted, across = pl["status"] == R.VOTED, (pl["e"] > plen) | (pl["q_end"] > plen)
    seen = dict(all_vote=bool(voted.all()), contained_across=bool((voted & across & (pl["anchor"] != R.NO)).sum() == 2), backbone_across=bool((voted & across & (pl["anchor"] == R.NO)).any()),
                tie=int(recs[int(pl[12]["anchor"])]["cid"]) == 1, doubled=int(pl[13]["band"]) == 512 and int(pl[12]["band"]) == 256 and bool(across[13]),
                orient1=bool((voted & across & (pl["orient"] == 1)).any()), orient0=bool((voted & across & (pl["orient"] == 0)).any()),
                shifted=bool((voted & (pl["s"] >= plen)).any()), begins_behind_the_seam=bool((voted & (pl["q_begin"] >= plen)).any()),
                spans_the_seam=bool((voted & (pl["q_begin"] < plen) & (pl["q_end"] > plen)).any()), wrapped=r["counts"]["wrapped"] == int((voted & across).sum()))
    assert all(seen.values()), seen
    plain = R.realign_round(u, p, seqs, recs, m["contained"], c["removed"], None, band0=256)
    assert np.flatnonzero(plain["placements"]["status"] == R.OUTSIDE).tolist() == [1, 2, 12]      # (read 13's forged window ends inside the line)


TRIM = dict(min_depth=1, end_clip=0, min_span=200)


def test_a_trim_in_force_on_the_circle():
    """circle_plus with 150 junk bases behind read 12: the trim clips them, the circle stays whole, and the clip votes across the origin"""
    seqs, recs = CC.circle_plus(junk=150)
    lens = np.array([len(s) for s in seqs])
    clip = TM.clips(recs, lens, **TRIM)
    assert (int(clip[12]["beg"]), int(clip[12]["end"]), int(lens[12])) == (0, 800, 950) and (clip["beg"][:12] == 0).all() and (clip["end"][:12] == 1500).all()
    g = TM.build(recs, lens, clip, **RC.GRAPH)
    c = U.clean(g["offsets"], g["edges"], g["contained"])
    u = U.unitigs(c["offsets"], c["edges"], g["contained"], c["removed"], g["lens"])
    assert u["circular"].tolist() == [1] and u["len"].tolist() == [6000]
    p = TM.polished(u, seqs, CC.gentle_table(seqs, 3), clip, 3)
    r = R.realign_round(u, p, seqs, recs, g["contained"], c["removed"], (clip["beg"], clip["end"]), band0=256, circular=True)
    pl = r["placements"]
    assert (pl["status"] == R.VOTED).all() and int(pl[12]["e"]) > len(p["bases"]) and int(pl[12]["n_eq"]) + int(pl[12]["n_x"]) + int(pl[12]["n_ins"]) == 800


def test_a_noisy_circle_gains_near_its_origin_and_loses_nothing_elsewhere():
    """30 x of 1.5 kb reads at 15 % error around 6 kb.  Windows of 400 bases from every backbone segment's start against their templates;
    a window is NEAR the origin when its segment starts within one read length of it, on either side.  Condition: the near windows' summed
    distance with the circle rule is BELOW the sum without it, and the far windows' sum is not above the plain sum by more than the far
    windows' own spread between the two runs (the sum of |difference| per window)."""
    W = 400
    x = CC.noisy_circle()
    u, pol, glen = x["u"], x["polished"], len(x["genome"])
    dbl = x["genome"] + x["genome"]
    args = (u, pol, x["seqs"], x["recs"], x["contained"], np.zeros(len(x["seqs"]), np.uint8), None)
    plain = R.realign_round(*args, band0=256)
    circ = R.realign_round(*args, band0=256, circular=True)
    assert circ["counts"]["outside"] == 0 and plain["counts"]["outside"] > 0 and circ["counts"]["voted"] > plain["counts"]["voted"] and circ["counts"]["wrapped"] > 0
    near, far, spread = [0, 0], [0, 0], 0
    for i, r in enumerate(x["chain"]):
        s = int(x["starts"][r])
        t = dbl[s:s + 5 * W // 4]
        d = []
        for res in (plain, circ):
            a = int(res["pos"][i])
            two = res["bases"] + res["bases"]                          # (a window of the last segment may run across the origin)
            d.append(U.window_distance(two[a:a + W], t))
        if s < 1500 or s >= glen - 1500:
            near[0] += d[0]; near[1] += d[1]
        else:
            far[0] += d[0]; far[1] += d[1]
            spread += abs(d[0] - d[1])
    print("REALIGN noisy circle: windows near the origin: plain %d, circular %d; elsewhere: plain %d, circular %d (spread %d); plain %s; circular %s"
          % (near[0], near[1], far[0], far[1], spread, plain["counts"], circ["counts"]))
    assert near[1] < near[0], near
    assert far[1] <= far[0] + spread, (far, spread)


def test_the_stats_and_the_new_entry_points_equal_the_header(tmp_path):
    """bella_realign_stats keeps its 176 bytes (`wrapped` has a getter of its own); the two new symbols are declared, exported and bound"""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bella_realign_stats));']
    for fname, _ in _lib.RealignStats._fields_:
        src.append('printf("%s %%zu\\n", offsetof(bella_realign_stats, %s));' % (fname, fname))
    src.append('printf("params %zu\\n", sizeof(bella_realign_params));')
    src.append('printf("placement %zu\\n", sizeof(bella_realign_placement));')
    src.append('printf("pad %zu\\n", offsetof(bella_realign_placement, pad));')
    src.append('printf("abi %d\\n", BELLA_HIP_ABI_VERSION);')
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    protos = tmp_path / "protos.c"
    protos.write_text('#include "bella_hip.h"\n'
                      'int (*run)(bella_ctx*, const bella_realign_params*, uint64_t*) = bella_hip_graph_realign_unitigs_circular;\n'
                      'int (*wr)(bella_ctx*, uint64_t*) = bella_hip_graph_get_realign_wrapped;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")])
    got = {a: int(v) for a, v in (ln.split() for ln in subprocess.check_output([exe]).decode().splitlines())}
    assert got["size"] == ctypes.sizeof(_lib.RealignStats) == 176
    for fname, _ in _lib.RealignStats._fields_:
        assert got[fname] == getattr(_lib.RealignStats, fname).offset, fname
    assert "wrapped" not in dict(_lib.RealignStats._fields_)
    assert got["params"] == ctypes.sizeof(_lib.RealignParams) == 24 and got["placement"] == _lib.PLACE_DT.itemsize == R.PLACE_DT.itemsize == 88
    assert got["pad"] == _lib.PLACE_DT.fields["pad"][1] == R.PLACE_DT.fields["pad"][1] and "pad" not in R.COMPARED
    assert got["abi"] == 6
    lib = _lib.load()
    assert lib.bella_hip_abi_version() == 6
    fn = lib.bella_hip_graph_realign_unitigs_circular                                     # exported and bound
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 3
    assert fn(None, None, None) == -3                                                      # BELLA_ERR_BAD_ARG without a context: no device is touched
    wr = lib.bella_hip_graph_get_realign_wrapped
    assert wr.restype is ctypes.c_int and len(wr.argtypes) == 2 and wr(None, None) == -3


def _cli():
    from bella_amd import build as b
    return b.build_cli()


def test_cli_lists_and_refuses_the_option_without_polish():
    p = subprocess.run([_cli(), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0 and "--realign-circular " in p.stdout.decode()
    for flags, word in ((["--unitigs", "u", "--realign-circular"], "--realign-circular needs --polish"),
                        (["--unitigs", "u", "--polish-rounds", "2", "--realign-circular"], "--realign-circular needs --polish"),
                        (["--unitigs", "u", "--polish", "--realign-circular=1"], "takes no value")):
        p = subprocess.run([_cli(), "-f", "none.txt", "-o", "none"] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and word in p.stderr.decode(), (flags, p.stderr)
