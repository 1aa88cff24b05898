"""GPU tests of the affine pair alignment: through bella_hip_align_sequences_affine the device result EQUALS the
mirror (bella_testkit/affine_mirror.py) in every field of every pair and, through op_off, in every run -- the three modes in the four
band classes; (1, 1, 0, 1) against the mirror and, byte for byte, against bella_hip_align_sequences; single gaps across lane and tile
seams; the band-doubling edges; the smallest inputs; the extremes of the scores; TOO_LARGE by the score bound and by the budget; the rc
flag; no pairs; bad scorings refused before anything is written; the getters after either call; evaluate.sequence_identity."""
import ctypes as C

import numpy as np
import pytest

from bella_amd import Engine, _lib, evaluate
from bella_testkit import affine_cases as FC
from bella_testkit import affine_mirror as FM
from bella_testkit import align_cases as AC
from bella_testkit import align_mirror as AM
from bella_testkit.pipeline import raises, with_round_budget

pytestmark = pytest.mark.gpu

BAD = -3
EDGES = AC.edge_cases()


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _records(case):
    return AM.records_of(case["seqs"], case["pairs"], case["mode"], case["rc"], case["centre"], case["overlap"])


def _same(eng, case, scoring, budget=None):
    """one affine call on the device against the mirror's: every compared field of every pair, every run, the counts; and every ALIGNED
    pair's runs are an alignment of its two sequences that re-scores to its score"""
    bases, recs = _records(case)
    got, ops = eng.align_records(bases, recs, case["mode"], case["band0"], case["band_max"], scoring=scoring)
    st = eng.align_stats()
    m = FM.align(bases, recs, case["mode"], case["band0"], case["band_max"], budget=budget, scoring=scoring)
    assert got.dtype == _lib.ALIGN_RES_DT == AM.RES_DT and ops.dtype == np.uint32
    for f in AM.COMPARED:
        assert np.array_equal(got[f], m["results"][f]), (f, got[f], m["results"][f])
    assert np.array_equal(ops, m["ops"])
    assert {k: st[k] for k in m["counts"]} == m["counts"] and st["mode"] == AM.MODES[case["mode"]]
    for rec, r in zip(recs, got):
        if int(r["status"]) == AM.ALIGNED:
            Q, T = AM.oriented(bases, rec)
            counts = FM.replay(ops[int(r["op_off"]):int(r["op_off"]) + int(r["nops"])], Q, T, r, scoring)
            assert counts == {f: int(r[f]) for f in ("n_eq", "n_x", "n_ins", "n_del", "score")}
        else:
            assert int(r["nops"]) == 0 and int(r["score"]) == 0
    return got, ops, st


# ---- modes and band classes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band0", [256, 512, 1024, 2048])
@pytest.mark.parametrize("mode", AC.MODES)
def test_every_mode_in_every_band_class_equals_the_mirror(eng, mode, band0):
    """pairs of 300 .. 700 bases at 10 % under (2, 4, 4, 2): first bands of 256, 512 and 1,024 (the three register kernels) and 2,048 (the
    wide one)"""
    got, _, st = _same(eng, AC.band_class_case(mode, band0), FC.MAIN)
    assert (got["status"] == AM.ALIGNED).all() and (got["band"] == band0).any() and st["batches"] >= 1 and st["dp_ms"] > 0
    assert (got["n_eq"] > 100).all()


# ---- two kernel families, one answer -----------------------------------------------------------------------------------------------------
def _linear_twice(eng, case):
    bases, recs = _records(case)
    _same(eng, case, FC.LINEAR)
    aff, aops = eng.align_records(bases, recs, case["mode"], case["band0"], case["band_max"], scoring=FC.LINEAR)
    lin, lops = eng.align_records(bases, recs, case["mode"], case["band0"], case["band_max"])
    assert aff.tobytes() == lin.tobytes() and aops.tobytes() == lops.tobytes()
    return aff


@pytest.mark.parametrize("name", sorted(EDGES))
def test_under_1_1_0_1_an_edge_case_equals_the_mirror_and_the_linear_call(eng, name):
    _linear_twice(eng, EDGES[name])


@pytest.mark.parametrize("mode", AC.MODES)
def test_under_1_1_0_1_mixed_lengths_equal_the_mirror_and_the_linear_call(eng, mode):
    got = _linear_twice(eng, AC.mixed_case(mode))
    assert (got["status"] == AM.ALIGNED).sum() >= 8


# ---- seams of the scan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["D", "I"])
@pytest.mark.parametrize("band0", [256, 512, 1024, 2048])
@pytest.mark.parametrize("mode", AC.MODES)
def test_a_single_gap_comes_back_as_one_run(eng, mode, band0, kind):
    """under (1, 3, 5, 1), a pair whose only difference is one gap: C + 1 bases (across a lane boundary) and 70 (across many lanes) in each
    register class, 300 (across a tile of 256 cells) in the wide sweep; 'D' runs along a row (F, the scan), 'I' down the rows (E)"""
    for length in FC.seam_lengths(band0):
        case, runs = FC.gap_case(mode, band0, length, kind)
        got, ops, _ = _same(eng, case, FC.GAPPY)
        r = got[0]
        assert ops.tolist() == runs, (length, ops)
        assert (int(r["status"]), int(r["band"]), int(r["score"])) == (AM.ALIGNED, band0, 400 - 5 - length)
        assert int(r["n_del" if kind == "D" else "n_ins"]) == length and int(r["n_eq"]) == 400 and int(r["nops"]) == 3


# ---- the band-doubling edges, the smallest inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in EDGES if n.startswith(("block_", "one_", "600_", "identical_", "nothing_", "dovetail_best"))))
def test_an_edge_case_under_2_4_4_2(eng, name):
    got, ops, st = _same(eng, EDGES[name], FC.MAIN)
    r = got[0]
    if name.startswith("block_120"):
        assert (int(r["status"]), int(r["band"]), st["repeated"], int(r["n_ins"])) == (AM.ALIGNED, 512, 1, 120)
        assert (ops & 15).tolist().count(2) == 1                       # one run of 'I'
    if name.startswith("block_248"):
        assert (int(r["status"]), int(r["band"])) == (AM.BAND_CAPPED, 512) and len(ops) == 0
    if name == "dovetail_best_cell_in_row_0":
        assert (int(r["status"]), int(r["nops"]), int(r["q_end"]), int(r["t_begin"])) == (AM.ALIGNED, 0, 0, 300) and len(ops) == 0
    if name == "one_base_match_global":
        assert (int(r["score"]), ops.tolist()) == (2, [1 << 4 | 0])
    if name == "one_base_mismatch_global":
        assert (int(r["score"]), ops.tolist()) == (-4, [1 << 4 | 1])
    if name == "identical_global":
        assert (int(r["score"]), ops.tolist()) == (1000, [500 << 4 | 0])


@pytest.mark.parametrize("scoring", FC.EXTREMES)
@pytest.mark.parametrize("mode", AC.MODES)
def test_the_extremes_of_the_scores(eng, mode, scoring):
    got, _, _ = _same(eng, FC.extreme_case(mode), scoring)
    assert (got["status"] == AM.ALIGNED).all()


# ---- TOO_LARGE ---------------------------------------------------------------------------------------------------------------------------
def test_too_large_by_the_score_bound_before_any_dp(eng):
    """2 x 263,200 bases under (1, 255, 0, 1): 526,400 * 255 >= 2^27; the same pair under (1, 1, 0, 1) would run"""
    half = 263_200
    bases = np.frombuffer(b"ACGT" * (half // 2), np.uint8)
    recs = np.zeros(2, AM.PAIR_DT)
    recs["q_off"], recs["t_off"], recs["q_len"], recs["t_len"] = [0, 0], [half, 100], [half, 100], [half, 100]
    got, ops = eng.align_records(bases, recs, "global", 256, 256, scoring=(1, 255, 0, 1))
    st = eng.align_stats()
    m = FM.align(bases, recs, "global", 256, 256, scoring=(1, 255, 0, 1))
    for f in AM.COMPARED:
        assert np.array_equal(got[f], m["results"][f]), f
    assert got["status"].tolist() == [AM.TOO_LARGE, AM.ALIGNED] and (int(got[0]["band"]), int(got[0]["score"])) == (256, 0)
    assert st["too_large"] == 1 and st["dp_cells"] == 100 * 256 and st["batches"] == 1 and np.array_equal(ops, m["ops"])
    assert not FM.too_large(half, half, FC.LINEAR)


@pytest.mark.parametrize("mode", AC.MODES)
def test_batches_under_a_round_budget(eng, mode):
    """BATCH_BUDGET holds one pair of about 500 rows at a band of 256 and 4 bits a cell: four batches or more, the same answers pair by
    pair wherever the pair still fits, and the pair of 2,000 rows is TOO_LARGE -- at 256 in the call, at 512 (2,000 * 256 bytes) alone"""
    case, alone = FC.budget_cases(mode)
    one, oops, ost = _same(eng, case, FC.MAIN)
    many, mops, mst = with_round_budget(eng, AC.BATCH_BUDGET, lambda: _same(eng, case, FC.MAIN, budget=AC.BATCH_BUDGET))
    assert mst["batches"] >= 4 and mst["batches"] > ost["batches"]
    assert int(many[5]["status"]) == AM.TOO_LARGE and int(many[5]["band"]) == 256 and int(one[5]["status"]) != AM.TOO_LARGE
    for k in range(13):
        if int(many[k]["status"]) == AM.TOO_LARGE:                     # (the mirror agreed: a pair that had to double to 512 needs 128,000 bytes there)
            continue
        for f in AM.COMPARED:
            if f != "op_off":
                assert one[k][f] == many[k][f], (k, f)
        a, b = one[k], many[k]
        assert np.array_equal(oops[int(a["op_off"]):int(a["op_off"]) + int(a["nops"])], mops[int(b["op_off"]):int(b["op_off"]) + int(b["nops"])]), k
    bases, recs = _records(case)
    want = FM.align(bases, recs, mode, case["band0"], case["band_max"], budget=AC.BATCH_BUDGET, scoring=FC.MAIN)["results"]
    doubled = {k for k in range(13) if (int(want[k]["status"]), int(want[k]["band"])) == (AM.TOO_LARGE, 512)}
    assert set(np.flatnonzero(many["status"] == AM.TOO_LARGE).tolist()) == {5} | doubled      # what was skipped: the mirror's TOO_LARGE pairs, no other
    assert all(int(one[k]["band"]) >= 512 for k in doubled) and (many["status"] != AM.TOO_LARGE).sum() >= 8
    got, _, st = with_round_budget(eng, AC.BATCH_BUDGET, lambda: _same(eng, alone, FC.MAIN, budget=AC.BATCH_BUDGET))
    assert (int(got[0]["status"]), int(got[0]["band"]), st["batches"]) == (AM.TOO_LARGE, 512, 0)


# ---- reverse complement, no pairs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", AC.MODES)
def test_the_rc_flag_gives_what_the_reverse_complemented_query_gives(eng, mode):
    flagged, plain = AC.rc_case(mode)
    a, aops, _ = _same(eng, flagged, FC.MAIN)
    b, bops, _ = _same(eng, plain, FC.MAIN)
    assert a.tobytes() == b.tobytes() and np.array_equal(aops, bops) and (a["status"] == AM.ALIGNED).all()


def test_no_pairs_launch_nothing(eng):
    _same(eng, AC.band_class_case("global", 256), FC.MAIN)            # (so that there are runs to forget)
    res, ops = eng.align_records(np.zeros(0, np.uint8), np.zeros(0, _lib.ALIGN_PAIR_DT), scoring=FC.MAIN)
    st = eng.align_stats()
    assert len(res) == 0 and len(ops) == 0
    assert (st["pairs"], st["batches"], st["dp_cells"], st["ops"], st["pack_ms"], st["dp_ms"], st["walk_ms"]) == (0, 0, 0, 0, 0, 0, 0)
    assert eng.lib.bella_hip_align_sequences_affine(eng.h, None, 0, None, 0, None, None, None, None) == 0      # the defaults; every pointer may be NULL


# ---- bad arguments -----------------------------------------------------------------------------------------------------------------------
def test_bad_scorings_are_refused_before_anything_is_written(eng):
    good = AC.band_class_case("global", 256)
    bases, recs = _records(good)
    kept, kops, _ = _same(eng, good, FC.MAIN)
    lib, h = eng.lib, eng.h
    recs = np.ascontiguousarray(recs, _lib.ALIGN_PAIR_DT)
    ap = _lib.AlignParams(C.sizeof(_lib.AlignParams), 0, 256, 4096)

    def call(sc, ap=ap):
        out = np.full(len(recs), 0xEE, np.uint8).repeat(_lib.ALIGN_RES_DT.itemsize).view(_lib.ALIGN_RES_DT)
        no = C.c_uint64(77)
        rc = lib.bella_hip_align_sequences_affine(h, bases.ctypes.data, bases.size, recs.ctypes.data, len(recs), C.byref(ap), C.byref(sc) if sc is not None else None,
                                                  out.ctypes.data, C.byref(no))
        return rc, out, no.value

    def refused(sc, ap=ap):
        rc, out, no = call(sc, ap)
        assert rc == BAD and out.tobytes() == b"\xee" * out.nbytes and no == 77      # nothing written
        ops = np.zeros(len(kops), np.uint32)
        assert lib.bella_hip_get_align_ops(h, ops.ctypes.data, len(ops)) == 0 and np.array_equal(ops, kops)      # the runs of the call before
        assert eng.align_stats()["ops"] == len(kops)
    size = C.sizeof(_lib.AlignScoring)
    refused(_lib.AlignScoring(size, 0, 4, 4, 2, 0))                    # match = 0
    refused(_lib.AlignScoring(size, 2, 4, 4, 0, 0))                    # gap_extend = 0
    for k in range(1, 5):                                              # a score of 256, in each place
        v = [2, 4, 4, 2]
        v[k - 1] = 256
        refused(_lib.AlignScoring(size, *v, 0))
    refused(_lib.AlignScoring(size, 2, 4, 4, 2, 1))                    # reserved = 1
    refused(_lib.AlignScoring(size - 4, 2, 4, 4, 2, 0))                # a struct_size too small
    refused(_lib.AlignScoring(size, 2, 4, 4, 2, 0), _lib.AlignParams(C.sizeof(_lib.AlignParams), 3, 256, 4096))      # and the other call's checks apply
    refused(_lib.AlignScoring(size, 2, 4, 4, 2, 0), _lib.AlignParams(C.sizeof(_lib.AlignParams), 0, 300, 4096))
    raises(BAD, lambda: eng.align_records(bases, recs, "global", 256, scoring=(0, 1, 1, 1)))
    rc, out, no = call(_lib.AlignScoring(size, 2, 4, 4, 2, 0))         # the good scoring, by hand
    assert rc == 0 and out.tobytes() == kept.tobytes() and no == len(kops)
    rc, out, no = call(None)                                           # scoring == NULL: (1, 1, 0, 1)
    want = FM.align(bases, recs, "global", 256, 4096, scoring=FC.LINEAR)
    assert rc == 0 and no == len(want["ops"]) and all(np.array_equal(out[f], want["results"][f]) for f in AM.COMPARED)

    class Longer(C.Structure):                                          # a later header's struct: eight more bytes
        _fields_ = _lib.AlignScoring._fields_ + [("more", C.c_uint64)]
    longer = Longer(C.sizeof(Longer), 2, 4, 4, 2, 0, 0)
    rc, out, no = call(C.cast(C.pointer(longer), C.POINTER(_lib.AlignScoring)).contents)
    assert rc == 0 and out.tobytes() == kept.tobytes()


# ---- the getters serve the last call -----------------------------------------------------------------------------------------------------
def test_a_linear_call_after_an_affine_one_and_the_reverse(eng):
    case = AC.band_class_case("semiglobal", 256)
    bases, recs = _records(case)

    def getters():
        st = eng.align_stats()
        ops = np.zeros(st["ops"], np.uint32)
        assert eng.lib.bella_hip_get_align_ops(eng.h, ops.ctypes.data, len(ops)) == 0
        return ops, st
    aff, aops = eng.align_records(bases, recs, "semiglobal", 256, scoring=FC.GAPPY)
    g, st = getters()
    assert np.array_equal(g, aops) and st["ops"] == len(aops)
    lin, lops = eng.align_records(bases, recs, "semiglobal", 256)
    g, st = getters()
    assert np.array_equal(g, lops) and not np.array_equal(lops, aops) and np.array_equal(lops, AM.align(bases, recs, "semiglobal", 256)["ops"])
    again, gops = eng.align_records(bases, recs, "semiglobal", 256, scoring=FC.GAPPY)
    g, st = getters()
    assert np.array_equal(g, aops) and np.array_equal(gops, aops) and again.tobytes() == aff.tobytes()


# ---- identity ----------------------------------------------------------------------------------------------------------------------------
def test_sequence_identity_under_a_scoring_equals_the_mirrors_counts(eng):
    """20 pairs of 2,000 bases with 0.2 % .. 4 % known edits under (2, 4, 4, 2): identity = n_eq / columns of the mirror's global alignment"""
    queries, templates, _ = AC.identity_case()
    ident, status = evaluate.sequence_identity(eng, queries, templates, scoring=FC.MAIN)
    bases, recs = AM.records_of(queries + templates, [(k, 20 + k) for k in range(20)], "global")
    m = FM.align(bases, recs, "global", scoring=FC.MAIN)["results"]
    cols = m["n_eq"].astype(np.int64) + m["n_x"] + m["n_ins"] + m["n_del"]
    assert (status == AM.ALIGNED).all() and np.array_equal(status, m["status"])
    assert np.array_equal(ident, m["n_eq"] / cols)
    assert ident[0] > 0.99 and ident[19] < ident[0]
