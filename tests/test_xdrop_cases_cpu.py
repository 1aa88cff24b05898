"""The sets of bella_testkit/xdrop_cases.py have the events they are for.  The mirror (bella_testkit/xdrop_mirror.py) equals the
oracle on every field of every pair of every set, so its traces speak for the oracle's extension too; every label then holds in the
trace: the X-drop on the step, in the phase, on the side and strand the label names, the end of Phase 2 on its step with the named
sequence ending, the kept direction on both sides of the boundary, the flank lengths, the places in the packed array.  So a failure
of tests/test_xdrop_edges_gpu.py on these sets is a failure of the kernels or of run_xdrop.

The int8 bounds: over all these inputs no saturation changes a value that was not at the bound already, and no rebase sees a
negative minimum (test_no_clamp_is_reached): the deferred upper clamp, the negative-minimum branch of the rebase and the lower
saturation of a live cell are not reached here -- an observation, with the argument that neighbouring cells differ by at most 3."""
import os

import numpy as np
import pytest

import _oracle as O
from bella_testkit import xdrop_cases as XC
from bella_testkit import xdrop_mirror as M
from conftest import ROOT, load_golden

FIELDS = ("score", "begH", "endH", "begV", "endV", "ov", "strand", "passed", "steps", "flagged")
S = XC.S
_records = {}
_mirrors = {}


def oracle_records(cs):
    """the oracle's answer on every seed of a case set, FIELDS per pair; computed once per set"""
    if cs.name not in _records:
        phi = O.slope(cs.err)
        out = np.zeros((len(cs.seeds), len(FIELDS)), np.int64)
        for n, (rid, cid, i, j) in enumerate(cs.seeds):
            e = O.xavier_align(cs.seqs[rid], cs.seqs[cid], i, j, cs.X, cs.k)
            ok, ov = O.post_align(e["score"], e["begV"], e["endV"], e["begH"], e["endH"], len(cs.seqs[rid]), len(cs.seqs[cid]), phi)
            out[n] = (e["score"], e["begH"], e["endH"], e["begV"], e["endV"], ov, e["strand"], int(ok), e["steps"], e["flagged"])
        out.setflags(write=False)
        _records[cs.name] = out
    return _records[cs.name]


def mirrored(cs, only=None):
    """the mirror on every seed of a case set (or on the seeds `only`) -- after it was held against the oracle on them"""
    key = (cs.name, None if only is None else tuple(only))
    if key not in _mirrors:
        seeds = cs.seeds if only is None else [cs.seeds[n] for n in only]
        res = M.align_many(cs.seqs, seeds, cs.k, cs.X, err=cs.err)
        exp = oracle_records(cs) if only is None else oracle_records(cs)[list(only)]
        got = np.array([[m[f] for f in FIELDS] for m in res], np.int64)
        for n in np.flatnonzero((got != exp).any(1)):
            raise AssertionError("%s pair %d %r: mirror %r, oracle %r" % (cs.name, n, cs.labels[n], got[n].tolist(), exp[n].tolist()))
        _mirrors[key] = res
    return _mirrors[key]


def four_ways(cs, res, **want):
    """the traces of the four pairs (two sides, two strands) whose label has `want`; each is the trace of the side it names"""
    out = []
    for side in XC.SIDES:
        for strand in XC.STRANDS:
            hit = [n for n, lab in enumerate(cs.labels) if all(lab.get(a) == b for a, b in dict(want, side=side, strand=strand).items())]
            assert len(hit) == 1, (cs.name, want, side, strand)
            m = res[hit[0]]
            assert m["strand"] == (strand == "c"), cs.labels[hit[0]]
            assert m[side]["ran"], cs.labels[hit[0]]
            out.append(m[side])
    return out


def test_slice_constant_is_the_one_the_cases_target():
    text = open(os.path.join(ROOT, "bella_amd", "csrc", "xdrop_packed.hpp")).read()
    assert XC.slice_default(text) == S == 512


def test_drop_in_phase2_around_the_boundaries():
    cs = XC.drop_set()
    res = mirrored(cs)
    assert len(cs.seeds) == 4 * len(XC.DROP_STEPS)
    for T in (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1):
        for t in four_ways(cs, res, event="drop_p2", step=T):
            assert (t["drop_step"], t["drop_phase"], t["steps"]) == (T, 2, T) and t["p2_end_step"] is None and not t["p1_drop"]


def test_phase2_ends_around_the_boundary_h_first_and_v_first():
    cs = XC.end_set()
    res = mirrored(cs)
    assert len(cs.seeds) == 4 * 2 * len(XC.END_STEPS)
    for first in "HV":
        for T in (S - 28, S - 27, S - 14, S - 1, S, S + 1):
            for t in four_ways(cs, res, event="p2_end", step=T, seq=first):
                assert (t["p2_end_step"], t["p2_end_seq"], t["p4_steps"], t["drop_step"]) == (T, first, 28, None)
                assert t["steps"] == T + 28


def test_drop_in_phase4_behind_the_boundary():
    cs = XC.tail_drop_set()
    res = mirrored(cs)
    for first in "HV":
        for t in four_ways(cs, res, event="drop_p4", seq=first):
            assert t["drop_phase"] == 4 and t["p2_end_seq"] == first and t["p2_end_step"] < S <= t["drop_step"]
            assert 0 < t["p4_steps"] < 28 and t["steps"] == t["drop_step"] == t["p2_end_step"] + t["p4_steps"]


@pytest.mark.parametrize("X", [100, 127])
def test_kept_direction_crosses_the_boundary(X):
    cs = XC.kept_set(X)
    res = mirrored(cs)
    assert cs.X == X
    for d in ("right", "down"):
        for t in four_ways(cs, res, event="kept", direction=d):
            assert (S - 1, d) in t["nonpos_steps"] and (S, d) in t["nonpos_steps"] and t["steps"] > S


def test_early_endings():
    cs = XC.early_set()
    res = mirrored(cs)
    for t in four_ways(cs, res, event="p1_drop"):
        assert t["p1_drop"] and t["steps"] == 0 and t["drop_step"] is None
    for t in four_ways(cs, res, event="first_step_drop"):
        assert not t["p1_drop"] and (t["drop_step"], t["drop_phase"], t["steps"]) == (0, 2, 0)
    for t in four_ways(cs, res, event="flagged"):
        assert t["flagged"] == 1 and t["steps"] > 0
    for t in four_ways(cs, res, event="clean"):
        assert t["drop_step"] is None and t["p4_steps"] == 28 and t["p2_end_step"] is not None and not t["flagged"]
    assert any(m["flagged"] for m in res)


def extension_lengths(cs, n):
    """(H, V) lengths the left and the right extension of seed n read, from the reads and the seed alone"""
    rid, cid, i, j = cs.seeds[n]
    lh, lv = len(cs.seqs[rid]), len(cs.seqs[cid])
    if cs.labels[n]["strand"] == "c":
        i = lh - i - cs.k
    return {"left": (i + cs.k, j + cs.k), "right": (lh - i - cs.k, lv - j - cs.k)}


def test_flank_lengths_on_both_sequences_sides_and_strands():
    cs = XC.flank_set()
    res = mirrored(cs)
    seen = set()
    for n, (lab, m) in enumerate(zip(cs.labels, res)):
        assert m["strand"] == (lab["strand"] == "c")
        lens = extension_lengths(cs, n)[lab["side"]]
        a, b = lens if lab["which"] == "H" else lens[::-1]
        assert (a, b) == (lab["length"], lab["partner"]), lab
        t, other = m[lab["side"]], m["left" if lab["side"] == "right" else "right"]
        assert t["ran"] == (a >= 32) and other["ran"], lab
        if t["ran"]:                                            # identical flanks: no drop, and the clearly shorter one runs out
            assert t["drop_step"] is None and t["p2_end_seq"] in "HV", lab
            if abs(a - b) > 16:
                assert t["p2_end_seq"] == (lab["which"] if a < b else "HV".replace(lab["which"], "")), lab
        elif lab["side"] == "right":                            # `beg` written where `end` was meant: the begin lies behind the end
            assert m["begH"] == len(cs.seqs[cs.seeds[n][0]]) > m["endH"] and m["begV"] == len(cs.seqs[cs.seeds[n][1]]) > m["endV"], lab
        else:
            assert (m["begH"], m["begV"]) == (0, 0), lab
        seen.add((lab["length"], lab["which"], lab["partner"], lab["side"], lab["strand"]))
    assert seen == {(a, w, p, s, st) for a in (31, 32, 33, 47, 48, 49, 63, 64, 65) for w in "HV" for p in (32, 300) for s in XC.SIDES for st in XC.STRANDS}


@pytest.mark.parametrize("total_mod", [0, 1, 15])
def test_places_in_the_packed_array(total_mod):
    cs = XC.place_set(total_mod)
    res = mirrored(cs)
    rs = cs.rs
    off, lens = rs.offsets, rs.lengths
    assert int(off[-1]) % 16 == total_mod
    tags = set()
    for n, (lab, m) in enumerate(zip(cs.labels, res)):
        rid, cid = cs.seeds[n][:2]
        assert m["strand"] == (lab["strand"] == "c"), lab
        if lab["event"] == "same_read":
            assert rid == cid == lab["read"] and m["left"]["ran"] and m["right"]["ran"]
            assert (m["begH"], m["begV"]) == (0, 0) or m["left"]["p2_end_step"] is not None
            tags.add(("same_read", lab["strand"]))
            continue
        r = lab["read"]
        assert (rid if lab["which"] == "H" else cid) == r
        for side in XC.SIDES:                                   # both extensions run on identical bases until the window ends
            t = m[side]
            assert t["ran"] and t["p2_end_seq"] == lab["which"] and t["drop_phase"] != 2, (lab, side)
        # ... so the window's first and last base are read: begin 0 and end = length (on the "c" strand H is read backwards)
        beg, end, ln = (m["begH"], m["endH"], int(lens[r])) if lab["which"] == "H" else (m["begV"], m["endV"], int(lens[r]))
        assert beg == 0 and end == ln, lab
        for tag in lab["tags"]:
            ok = {"first_read": r == 0 and off[r] == 0, "start0": off[r] % 16 == 0 and r > 0, "start1": off[r] % 16 == 1,
                  "start15": off[r] % 16 == 15, "short_pred": r > 0 and lens[r - 1] < 16,
                  "last_read": r == rs.nreads - 1}[tag]
            assert ok, lab
            tags.add((tag, lab["which"], lab["strand"]))
    want = {(t, w, s) for t in ("first_read", "start0", "start1", "start15", "short_pred", "last_read") for w in "HV" for s in XC.STRANDS}
    assert tags == want | {("same_read", "n"), ("same_read", "c")}
    assert {int(lens[r - 1]) for lab in cs.labels if "short_pred" in lab.get("tags", ()) for r in [lab["read"]]} == {7, 15}


@pytest.mark.parametrize("k", XC.KS)
@pytest.mark.parametrize("X", XC.XS)
def test_mixed_set_under_every_k_and_x(k, X):
    cs = XC.mixed_set(k, X)
    res = mirrored(cs)
    assert len(res) == 300
    kinds = {(lab["noise"], lab["strand"]) for lab in cs.labels}
    assert kinds == {(z, s) for z in XC.NOISE for s in XC.STRANDS}
    for lab, m in zip(cs.labels, res):
        assert m["strand"] == (lab["strand"] == "c"), lab
    assert sum(len(cs.seqs[r]) != len(cs.seqs[c]) for r, c, _, _ in cs.seeds) > 100
    if X >= 60:                                                  # most extensions that run cross a boundary, many cross two
        ran = [t for m in res for t in (m["left"], m["right"]) if t["ran"]]
        assert sum(t["steps"] >= S for t in ran) * 2 > len(ran)
        assert sum(t["steps"] >= 2 * S for t in ran) * 8 > len(ran)


SAMPLE = 100


def survivor_sample():
    cs = XC.survivor_set()
    return list(range(0, len(cs.seeds), len(cs.seeds) // SAMPLE))[:SAMPLE]


def test_survivor_set_keeps_more_than_4096_alive_over_four_launches():
    cs = XC.survivor_set()
    exp = oracle_records(cs)
    steps = exp[:, FIELDS.index("steps")]
    good = np.array([lab["event"] == "survivor" for lab in cs.labels])
    assert int(good.sum()) == XC.SURVIVOR_SEEDS and int((~good).sum()) == XC.SURVIVOR_JUNK and len(cs.seeds) == 2450
    assert steps[~good].max() < S                                # the junk ends in the first launch, both extensions together
    # The oracle gives a pair's steps as the sum of its two extensions'.  An extension on sequences of a and b bases takes at most
    # (a - 30) + (b - 30) steps of Phase 2 and 28 of Phase 4, so each extension has at least the sum less the other one's bound.
    alive = 0
    for n in np.flatnonzero(good):
        ln = extension_lengths(cs, n)
        bound = {side: ln[side][0] + ln[side][1] - 60 + 28 for side in XC.SIDES}
        alive += int(steps[n]) - bound["right"] > 4 * S
        alive += int(steps[n]) - bound["left"] > 4 * S
    assert alive >= 4097
    # and the mirror has the two apart, on a sample
    pick = survivor_sample()
    for n, m in zip(pick, mirrored(cs, only=pick)):
        if good[n]:
            assert m["left"]["steps"] > 4 * S and m["right"]["steps"] > 4 * S and m["left"]["steps"] + m["right"]["steps"] == steps[n]
    assert {lab["strand"] for lab in cs.labels if lab["event"] == "survivor"} == {"n", "c"}


def golden_case(name):
    g = load_golden(name)
    Bc, Br, Bv = O.build_B(g.rs.nreads, g.tk, g.tr, g.tp)
    _, _, pairs = O.spgemm(g.seqs, g.nkmers, Bc, Br, Bv, g.k)
    seeds = [(int(p["rid"]), int(p["cid"]), int(p["seedH"]), int(p["seedV"])) for p in pairs[:300]]
    return XC.CaseSet("golden-" + name, g.k, g.xdrop, g.seqs, seeds, [{}] * len(seeds), err=g.err)


@pytest.mark.parametrize("name", ["toy120", "toyjunk220"])
def test_mirror_equals_oracle_on_golden_candidate_pairs(name):
    cs = golden_case(name)
    assert len(cs.seeds) == 300 and len(mirrored(cs)) == 300


def test_no_clamp_is_reached():
    """every trace of this file: every pair of every set and of the golden sets' first 300, the survivor set's sample"""
    sets = XC.small_sets() + [XC.mixed_set(k, X) for k in XC.KS for X in XC.XS] + [golden_case("toy120"), golden_case("toyjunk220")]
    runs = [mirrored(cs) for cs in sets] + [mirrored(XC.survivor_set(), only=survivor_sample())]
    ext = steps = rebases = 0
    worst_min, worst_span = 10 ** 9, 0
    for res in runs:
        for m in res:
            for t in (m["left"], m["right"]):
                if not t["ran"]:
                    continue
                ext += 1
                steps += t["steps"]
                assert t["hi_clamps"] == 0 and t["lo_clamps"] == 0
                for _, mn, span in t["rebases"]:
                    rebases += 1
                    worst_min, worst_span = min(worst_min, mn), max(worst_span, span)
    print("extensions %d, steps %d, rebases %d, smallest rebase minimum %d, largest max - min %d" % (ext, steps, rebases, worst_min, worst_span))
    assert rebases > 1000 and worst_min >= 0
