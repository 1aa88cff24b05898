"""GPU tests of the pair alignment: the device result EQUALS the mirror (bella_testkit/align_mirror.py) in every
field of every pair and, through op_off, in every run, on the inputs of bella_testkit/align_cases.py -- the three modes in the four
band classes, the edges, the reverse-complement flag, reuse and order, batches under BELLA_TUNE_ROUND_BUDGET; the call leaves the
context's stages alone; bad arguments are refused before anything is written; evaluate.sequence_identity."""
import ctypes as C

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib, api, evaluate
from bella_testkit import align_cases as AC
from bella_testkit import align_mirror as AM
from bella_testkit.pipeline import aligned, raises, with_round_budget
from conftest import load_golden

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


def _same(eng, case, budget=None):
    """one call on the device against the mirror's: every field of every pair, every run, the counts; and every ALIGNED pair's runs are
    an alignment of its two sequences"""
    bases, recs = _records(case)
    got, ops = eng.align_records(bases, recs, case["mode"], case["band0"], case["band_max"])
    st = eng.align_stats()
    m = AM.align(bases, recs, case["mode"], case["band0"], case["band_max"], budget=budget)
    assert got.dtype == _lib.ALIGN_RES_DT == AM.RES_DT and ops.dtype == np.uint32
    for f in AM.COMPARED:
        assert np.array_equal(got[f], m["results"][f]), (f, got[f], m["results"][f])
    assert np.array_equal(ops, m["ops"])
    assert {k: st[k] for k in m["counts"]} == m["counts"] and st["mode"] == AM.MODES[case["mode"]]
    for rec, r in zip(recs, got):
        if int(r["status"]) == AM.ALIGNED:
            Q, T = AM.oriented(bases, rec)
            counts = AM.replay(ops[int(r["op_off"]):int(r["op_off"]) + int(r["nops"])], Q, T, r)
            assert counts == {f: int(r[f]) for f in ("n_eq", "n_x", "n_ins", "n_del", "score")}
        else:
            assert int(r["nops"]) == 0 and int(r["score"]) == 0
    return got, ops, st


# ---- modes and band classes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band0", [256, 512, 1024, 2048])
@pytest.mark.parametrize("mode", AC.MODES)
def test_every_mode_in_every_band_class_equals_the_mirror(eng, mode, band0):
    """pairs of 300 .. 700 bases with 10 % substitutions and indels, first bands of 256, 512 and 1,024 (the three register kernels) and
    2,048 (the wide one, 600 rows)"""
    got, _, st = _same(eng, AC.band_class_case(mode, band0))
    assert (got["status"] == AM.ALIGNED).all() and (got["band"] == band0).any() and st["batches"] >= 1 and st["dp_ms"] > 0
    assert (got["n_eq"] > 100).all()


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EDGES))
def test_an_edge_case_equals_the_mirror(eng, name):
    got, ops, st = _same(eng, EDGES[name])
    r = got[0]
    if name == "global_start_outside_the_first_band":
        assert (int(r["status"]), int(r["band"]), int(r["widened"]), st["repeated"]) == (AM.ALIGNED, 512, 1, 0)
    if name == "global_capped_before_any_dp":
        assert int(r["status"]) == AM.BAND_CAPPED and st["batches"] == 0 and st["dp_cells"] == 0
    if name.startswith("block_120"):
        assert (int(r["status"]), int(r["band"]), st["repeated"], int(r["n_ins"])) == (AM.ALIGNED, 512, 1, 120)
    if name.startswith("block_248"):
        assert (int(r["status"]), int(r["band"])) == (AM.BAND_CAPPED, 512) and len(ops) == 0
    if name == "dovetail_best_cell_in_row_0":
        assert (int(r["status"]), int(r["nops"]), int(r["q_end"]), int(r["t_begin"])) == (AM.ALIGNED, 0, 0, 300) and len(ops) == 0


# ---- reverse complement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", AC.MODES)
def test_the_rc_flag_gives_what_the_reverse_complemented_query_gives(eng, mode):
    flagged, plain = AC.rc_case(mode)
    a, aops, _ = _same(eng, flagged)
    b, bops, _ = _same(eng, plain)
    assert a.tobytes() == b.tobytes() and np.array_equal(aops, bops) and (a["status"] == AM.ALIGNED).all()


# ---- reuse and order -------------------------------------------------------------------------------------------------------------------------
def test_one_sequence_used_by_50_pairs_in_shuffled_order(eng):
    case = AC.reuse_case()
    got, ops, _ = _same(eng, case)
    assert (got["status"] == AM.ALIGNED).all()
    # the wrapper builds the same records, and the answer belongs to the pair, not to its place in the call
    res, wops = eng.align_sequences(case["seqs"], case["pairs"], "semiglobal", rc=case["rc"], centre=case["centre"], band0=case["band0"])
    assert res.tobytes() == got.tobytes() and np.array_equal(wops, ops)
    back = np.argsort([q for q, _ in case["pairs"]])
    straight = dict(case, pairs=[case["pairs"][i] for i in back], rc=[case["rc"][i] for i in back], centre=[case["centre"][i] for i in back])
    sgot, sops, _ = _same(eng, straight)
    for f in AM.COMPARED:
        if f != "op_off":
            assert np.array_equal(sgot[f], got[f][back]), f
    for a, b in zip(sgot, got[back]):
        assert np.array_equal(sops[int(a["op_off"]):int(a["op_off"]) + int(a["nops"])], ops[int(b["op_off"]):int(b["op_off"]) + int(b["nops"])])
    cig = api.align_cigars(got, ops)
    assert all(c is not None and c for c in cig) and api.align_cigars(got, ops, eqx=False)[0].count(b"=") == 0


@pytest.mark.parametrize("mode", AC.MODES)
def test_mixed_lengths_in_one_call(eng, mode):
    """1 .. 2,000 bases with the wrapper's default centres: several bands in one call, the runs laid out by band, then by index"""
    case = AC.mixed_case(mode)
    got, _, st = _same(eng, case)
    res, _ = eng.align_sequences(case["seqs"], case["pairs"], mode, overlap=case["overlap"], band0=case["band0"])
    assert res.tobytes() == got.tobytes()
    assert st["aligned"] >= 8 and (mode != "global" or (len(set(got["band"].tolist())) >= 2 and st["repeated"] >= 1))


def test_no_pairs_launch_nothing(eng):
    _same(eng, AC.band_class_case("global", 256))                      # (so that there are runs to forget)
    res, ops = eng.align_records(np.zeros(0, np.uint8), np.zeros(0, _lib.ALIGN_PAIR_DT))
    st = eng.align_stats()
    assert len(res) == 0 and len(ops) == 0
    assert (st["pairs"], st["batches"], st["dp_cells"], st["ops"], st["pack_ms"], st["dp_ms"], st["walk_ms"]) == (0, 0, 0, 0, 0, 0, 0)
    assert eng.lib.bella_hip_align_sequences(eng.h, None, 0, None, 0, None, None, None) == 0      # the defaults; every pointer may be NULL


# ---- batching ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", AC.MODES)
def test_batches_under_a_round_budget(eng, mode):
    """BATCH_BUDGET holds three pairs of about 500 rows at a band of 256: four batches or more, the same answers pair by pair, and the
    pair of 2,000 rows is TOO_LARGE while the others stay aligned"""
    case = AC.batch_case(mode)
    one, oops, ost = _same(eng, case)
    many, mops, mst = with_round_budget(eng, AC.BATCH_BUDGET, lambda: _same(eng, case, budget=AC.BATCH_BUDGET))
    assert mst["batches"] >= 3 and mst["batches"] > ost["batches"]
    assert (many["status"] == AM.TOO_LARGE).tolist() == [k == 5 for k in range(13)] and int(one[5]["status"]) != AM.TOO_LARGE
    assert mst["too_large"] == 1 and mst["aligned"] == ost["aligned"] - int(one[5]["status"] == AM.ALIGNED)
    for k in range(13):
        if k == 5:
            continue
        for f in AM.COMPARED:
            if f != "op_off":
                assert one[k][f] == many[k][f], (k, f)
        a, b = one[k], many[k]
        assert np.array_equal(oops[int(a["op_off"]):int(a["op_off"]) + int(a["nops"])], mops[int(b["op_off"]):int(b["op_off"]) + int(b["nops"])]), k


# ---- state -------------------------------------------------------------------------------------------------------------------------------------
def _snapshot(eng):
    """what every getter of the stages returns, as bytes"""
    lib, h = eng.lib, eng.h
    out = {}

    def put(name, *arrays):
        out[name] = b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)
    put("reads", *eng.read_bases())
    put("pairs", *eng.get_pairs())
    put("alns", eng.get_alignments())
    ts = eng.trace_stats()
    tr, tops = np.zeros(eng.npairs, _lib.TRACE_DT), np.zeros(ts.ops, np.uint32)
    assert lib.bella_hip_get_traces(h, tr.ctypes.data, tops.ctypes.data if len(tops) else None) == 0
    put("traces", tr, tops)
    put("records", eng.graph_overlaps())
    put("graph", *eng.graph())
    put("removed", eng.graph_removed())
    us = eng.unitig_stats()
    u = [np.zeros(us["unitigs"] + 1, np.uint64), np.zeros(us["vertices"], np.uint32), np.zeros(us["vertices"], np.uint64), np.zeros(us["vertices"], np.uint32),
         np.zeros(us["unitigs"], np.uint64), np.zeros(us["unitigs"], np.uint8), np.zeros(us["links"], _lib.LINK_DT)]
    assert lib.bella_hip_graph_get_unitigs(h, *(a.ctypes.data if a.size else None for a in u)) == 0
    put("unitigs", *u)
    put("unitig_bases", *eng.unitig_bases())
    ps = eng.polish_stats()
    p = [np.zeros(ps["unitigs"] + 1, np.uint64), np.zeros(ps["bases_after"], np.uint8), np.zeros(ps["vertices"], np.uint64), np.zeros(ps["vertices"], np.uint32),
         np.zeros(ps["unitigs"], _lib.POLISH_DT)]
    assert lib.bella_hip_graph_get_polished(h, *(a.ctypes.data if a.size else None for a in p)) == 0
    put("polish", *p)
    put("pileup", eng.get_pileup())
    r = eng.realigned()
    put("realigned", *(r[k] for k in sorted(r) if isinstance(r[k], np.ndarray)))
    put("placements", eng.realign_placements())
    put("links", *eng.link_alignments())
    timers = lambda d: {k: v for k, v in d.items() if not k.endswith("_ms")}
    out["stats"] = repr([timers(eng.graph_stats()), timers(us), timers(ps), timers(eng.realign_stats()), timers(eng.link_stats()), ts.ops, ts.pairs])
    return out


def test_the_call_leaves_every_stage_as_it_found_it():
    """a context that holds reads, pairs, alignments, traces, a pileup, records, a cleaned graph, unitigs, a polish, a realignment round and
    aligned links: every getter returns the same bytes before and after a call, and a call on an empty context needs no reads"""
    e = Engine(0)
    try:
        case = AC.band_class_case("semiglobal", 256)
        bases, recs = _records(case)
        first, fops = e.align_records(bases, recs, "semiglobal", 256)          # a context without reads
        g = load_golden("toy120")
        pars, _, _ = aligned(e, g)
        e.pileup_reset()
        e.trace_pairs(pars, pileup=True)
        e.graph_reset()
        assert e.graph_add_traced() > 0
        e.graph_build(min_overlap=0, fuzz=10)
        e.graph_clean()
        assert len(e.graph_unitigs()["len"]) >= 1
        e.graph_polish_unitigs(3)
        e.graph_realign_unitigs()
        e.graph_align_links()
        before = _snapshot(e)
        for mode in AC.MODES:
            _same(e, AC.band_class_case(mode, 256))
        again, aops = e.align_records(bases, recs, "semiglobal", 256)
        assert again.tobytes() == first.tobytes() and np.array_equal(aops, fops)
        after = _snapshot(e)
        assert before.keys() == after.keys()
        for k in before:
            assert before[k] == after[k], k
        e.graph_polish_unitigs(3)                                       # and the stages go on from where they were
    finally:
        e.close()


# ---- bad arguments ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_written(eng):
    good = AC.band_class_case("global", 256)
    bases, recs = _records(good)
    kept, kops, _ = _same(eng, good)
    lib, h = eng.lib, eng.h

    def refused(bases, recs, mode=0, band0=256, band_max=4096, size=C.sizeof(_lib.AlignParams)):
        recs = np.ascontiguousarray(recs, _lib.ALIGN_PAIR_DT)
        out = np.full(len(recs), 0xEE, np.uint8).repeat(_lib.ALIGN_RES_DT.itemsize).view(_lib.ALIGN_RES_DT)
        ap = _lib.AlignParams(size, mode, band0, band_max)
        no = C.c_uint64(77)
        assert lib.bella_hip_align_sequences(h, bases.ctypes.data, bases.size, recs.ctypes.data, len(recs), C.byref(ap), out.ctypes.data, C.byref(no)) == BAD
        assert out.tobytes() == b"\xee" * out.nbytes and no.value == 77            # nothing written
        ops = np.zeros(len(kops), np.uint32)
        assert lib.bella_hip_get_align_ops(h, ops.ctypes.data, len(ops)) == 0 and np.array_equal(ops, kops)      # the runs of the call before
        assert eng.align_stats()["ops"] == len(kops)

    def changed(k, **fields):
        r = recs.copy()
        for f, v in fields.items():
            r[k][f] = v
        return r
    lower = bases.copy()
    lower[int(recs[1]["t_off"]) + 5] = ord("a")
    refused(lower, recs)                                               # a byte other than ACGT inside a used window
    enn = bases.copy()
    enn[int(recs[2]["q_off"])] = ord("N")
    refused(enn, recs)
    unused = np.concatenate([bases, np.frombuffer(b"NNNN", np.uint8)])  # ... but not outside every window
    got, gops = eng.align_records(unused, recs, "global", 256)
    assert got.tobytes() == kept.tobytes() and np.array_equal(gops, kops)
    refused(bases, changed(0, q_off=len(bases) - 3))                   # a window outside bases
    refused(bases, changed(3, t_off=len(bases)))
    refused(bases, changed(1, t_off=2 ** 63))
    refused(bases, changed(0, q_len=0))                                # a length of zero
    refused(bases, changed(2, t_len=0))
    refused(bases, changed(1, q_len=1 << 30))                          # a sequence of 2^30 bases or more
    refused(bases, changed(1, flags=2))
    refused(bases, recs, mode=3)
    for band0, band_max in ((300, 4096), (128, 4096), (1024, 512), (256, 32768), (256, 3000)):
        refused(bases, recs, band0=band0, band_max=band_max)
    refused(bases, recs, size=C.sizeof(_lib.AlignParams) - 4)           # a struct_size too small
    out = np.zeros(len(recs), _lib.ALIGN_RES_DT)
    assert lib.bella_hip_align_sequences(h, bases.ctypes.data, bases.size, recs.ctypes.data, len(recs), None, None, None) == BAD      # no room for the results
    assert lib.bella_hip_align_sequences(None, bases.ctypes.data, bases.size, recs.ctypes.data, len(recs), None, out.ctypes.data, None) == BAD
    raises(BAD, lambda: eng.align_records(bases, recs, mode=7))
    assert lib.bella_hip_get_align_ops(h, None, 0) == (BAD if len(kops) else 0)

    class Longer(C.Structure):                                          # a later header's struct: eight more bytes, all zero; zero bands are the defaults
        _fields_ = _lib.AlignParams._fields_ + [("more", C.c_uint64)]
    longer = Longer(C.sizeof(Longer), 0, 0, 0, 0)
    assert lib.bella_hip_align_sequences(h, bases.ctypes.data, bases.size, recs.ctypes.data, len(recs), C.cast(C.byref(longer), C.POINTER(_lib.AlignParams)), out.ctypes.data, None) == 0
    want = AM.align(bases, recs, "global", 512, 4096)["results"]
    assert all(np.array_equal(out[f], want[f]) for f in AM.COMPARED)
    buf = (C.c_uint8 * 16)(*([0xEE] * 16))                              # a caller with an older, shorter stats struct: only its bytes are written
    assert lib.bella_hip_get_align_stats(h, buf, 8) == 0
    assert bytes(buf[:8]) == len(recs).to_bytes(8, "little") and bytes(buf[8:]) == b"\xee" * 8


# ---- identity ----------------------------------------------------------------------------------------------------------------------------------
def test_sequence_identity_equals_the_mirrors_counts(eng):
    """20 pairs of 2,000 bases with 0.2 % .. 4 % known edits: identity = n_eq / columns of the mirror's global alignment, and no pair
    scores below the alignment that the edits themselves are"""
    queries, templates, edits = AC.identity_case()
    ident, status = evaluate.sequence_identity(eng, queries, templates)
    bases, recs = AM.records_of(queries + templates, [(k, 20 + k) for k in range(20)], "global")
    m = AM.align(bases, recs, "global")["results"]
    cols = m["n_eq"].astype(np.int64) + m["n_x"] + m["n_ins"] + m["n_del"]
    assert (status == AM.ALIGNED).all() and np.array_equal(status, m["status"])
    assert np.array_equal(ident, m["n_eq"] / cols)
    for k, (s, i, d) in enumerate(edits):                             # the edits that were made are an alignment: 2,000 - s - d matches, s + i + d others
        assert int(m[k]["score"]) >= 2000 - 2 * s - 2 * d - i, k
    assert ident[0] > 0.99 and ident[19] < ident[0]
    _, status = evaluate.sequence_identity(eng, queries, templates, mode="semiglobal", band0=256)
    assert (status == AM.ALIGNED).all()
