"""GPU tests of the circular realignment round: the device result EQUALS the mirror (bella_testkit/realign_mirror.py
with circular=True) -- placements with their pad word, alignment records, runs, table, bases, pos / nbases, counts with `wrapped` -- on the
circles of bella_testkit/realign_cases.py and realign_circle_cases.py under four band settings, over two rounds, in many batches (BELLA_TUNE_ROUND_BUDGET) and with a trim in
force; nothing else moves: a line, a circle that is too short for band_max and the plain entry point give what they gave; state and
errors of the new entry point; and bella-hip --realign-circular end to end on a noisy circle of 48 kb."""
import ctypes as C

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib
from bella_testkit import realign_cases as RC
from bella_testkit import realign_circle_cases as CC
from bella_testkit import realign_mirror as R
from bella_testkit import synth
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import dps_and_largest_job, raises, realign_getters, run_cli, same_but_for_the_batching, with_round_budget

pytestmark = pytest.mark.gpu

BANDS = {"b256": dict(band0=256), "b512": dict(band0=512, band_max=512), "b1024": dict(band0=1024), "b2048": dict(band0=2048)}
CASES = {"circle": RC.circle_case, "circle_plus": CC.circle_plus}
SEEN = dict(dp4=False, dp8_doubled=False, dp8=False, dp16=False, wide=False, contained_across=False, orient1_across=False, shifted=False, begins_behind_the_seam=False,
            spans_the_seam=False, trim=False)
TRIM = dict(min_depth=1, end_clip=0, min_span=200)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _install(eng, seqs, recs, graph, trim=None):
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_add_overlaps(recs)
    if trim is not None:
        eng.graph_trim(**trim)
    eng.graph_build(**graph)
    eng.graph_clean()
    return eng.graph_unitigs()


def _polish(eng, table, md=3):
    eng.pileup_reset()
    if table is not None:
        eng.add_pileup(0, eng.nreads, table)
    return eng.graph_polish_unitigs(md)


def _getters(eng):
    ops, table = eng.realign_ops()
    st = eng.realign_stats()
    return eng.realigned(), eng.realign_placements(), ops, table, {k: v for k, v in st.items() if not k.endswith("_ms")}


def _same(eng, u, cur, seqs, recs, clips=None, circular=True, **params):
    """one round on the device against the mirror's round on `cur`: -> (device result, mirror result, placements)"""
    got = eng.graph_realign_unitigs(circular=circular, keep_ops=1, **params)
    cont, rem = eng.graph()[2], eng.graph_removed()
    m = R.realign_round(u, cur, seqs, recs, cont, rem, clips, circular=circular, **{**R.DEFAULTS, **params})
    pl = eng.realign_placements()
    assert pl.dtype == _lib.PLACE_DT == R.PLACE_DT
    for f in R.COMPARED + ("pad",):
        assert np.array_equal(pl[f], m["placements"][f]), (f, pl[f], m["placements"][f])
    ops, table = eng.realign_ops()
    for r in np.flatnonzero(pl["status"] == R.VOTED).tolist():
        assert np.array_equal(ops[int(pl[r]["op_off"]):int(pl[r]["op_off"]) + int(pl[r]["nops"])], m["ops"][r]), r
    assert len(ops) == sum(len(x) for x in m["ops"].values())
    assert np.array_equal(table, m["table"])
    assert got["offsets"].dtype == np.uint64 and np.array_equal(got["offsets"], m["offsets"])
    assert got["bases"].tobytes() == m["bases"]
    assert got["pos"].dtype == np.uint64 and np.array_equal(got["pos"], m["pos"])
    assert got["nbases"].dtype == np.uint32 and np.array_equal(got["nbases"], m["nbases"])
    for f in U.POLISH_DT.names:
        assert np.array_equal(got["stats"][f], m["stats"][f]), f
    st = eng.realign_stats()
    want = dict(m["counts"], bases_before=int(cur["offsets"][-1]), bases_after=len(m["bases"]))
    want.setdefault("wrapped", 0)
    for f in ("substituted", "deleted", "inserted"):
        want[f] = int(m["stats"][f].sum())
    assert {k: st[k] for k in want} == want
    return got, m, pl


@pytest.mark.parametrize("bands", list(BANDS))
@pytest.mark.parametrize("case", list(CASES))
def test_the_circles_equal_the_mirror(eng, case, bands):
    """the circle and the circle with its two contained reads, polished with the gentle table: k_rea_dp<4> doubling to <8>, <8> alone, <16>
    and the wide kernel"""
    seqs, recs = CASES[case]()
    u = _install(eng, seqs, recs, RC.GRAPH)
    assert u["circular"].tolist() == [1] and u["len"].tolist() == [6000]
    p = _polish(eng, CC.gentle_table(seqs, 3))
    plen = len(p["bases"])
    assert plen != 6000
    got, m, pl = _same(eng, u, p, seqs, recs, **BANDS[bands])
    st = eng.realign_stats()
    print("REALIGN circular %s %s: %s; place %.3f ms, dp %.3f ms, walk %.3f ms, vote %.3f ms" % (case, bands, m["counts"], st["place_ms"], st["dp_ms"], st["walk_ms"], st["vote_ms"]))
    voted = pl["status"] == R.VOTED
    assert voted.all() and (pl["pad"] == 1).all() and st["outside"] == 0 and st["wrapped"] == int((voted & ((pl["e"] > plen) | (pl["q_end"] > plen))).sum()) > 0
    across = voted & (pl["q_end"] > plen)
    SEEN["dp4"] |= bool((voted & (pl["band"] == 256)).any())
    SEEN["dp8_doubled"] |= bands == "b256" and bool((across & (pl["band"] == 512)).any())
    SEEN["dp8"] |= bands == "b512" and bool((across & (pl["band"] == 512)).any())
    SEEN["dp16"] |= bool((across & (pl["band"] == 1024)).any())
    SEEN["wide"] |= bool((across & (pl["band"] == 2048)).any())
    SEEN["contained_across"] |= bool((across & (pl["anchor"] != R.NO)).any())
    SEEN["orient1_across"] |= bool((across & (pl["orient"] == 1)).any())
    SEEN["shifted"] |= bool((voted & (pl["s"] >= plen)).any())
    SEEN["begins_behind_the_seam"] |= bool((voted & (pl["q_begin"] >= plen)).any())
    SEEN["spans_the_seam"] |= bool((voted & (pl["q_begin"] < plen) & (pl["q_end"] > plen)).any())


@pytest.mark.parametrize("bands", ["b256", "b2048"])
def test_the_circle_in_one_job_per_batch(eng, bands):
    """circle_plus with round_budget = 1 against the default budget: the jobs on the unrolled circle (`pad`, the doubled pack) go through
    the batches one at a time -- k_rea_dp<4> doubling to <8>, and the wide kernel -- and everything comes out the same"""
    seqs, recs = CC.circle_plus()
    got = []
    for budget in (None, 1):
        _install(eng, seqs, recs, RC.GRAPH)
        _polish(eng, CC.gentle_table(seqs, 3))
        got.append(with_round_budget(eng, budget, lambda: realign_getters(eng, circular=True, keep_ops=1, **BANDS[bands])))
    one, many = got
    same_but_for_the_batching(one, many)
    pl = many["placements"]
    assert (pl["status"] == R.VOTED).all() and (pl["pad"] == 1).all() and many["st"]["wrapped"] > 0
    ndp, largest = dps_and_largest_job(pl["band"], [len(s) for s in seqs], BANDS[bands]["band0"])
    print("REALIGN circular circle_plus %s: %d batches by default, %d with one job per batch" % (bands, one["st"]["batches"], many["st"]["batches"]))
    assert many["st"]["batches"] == ndp > one["st"]["batches"] and many["st"]["dir_bytes_peak"] == largest


def test_two_rounds_equal_the_mirrors_two_rounds(eng):
    seqs, recs = CC.circle_plus()
    u = _install(eng, seqs, recs, RC.GRAPH)
    p = _polish(eng, CC.gentle_table(seqs, 3))
    got, m, _ = _same(eng, u, p, seqs, recs, band0=256)
    assert eng.realign_stats()["round"] == 1
    got2, m2, _ = _same(eng, u, m, seqs, recs, band0=256)
    assert eng.realign_stats()["round"] == 2 and eng.realign_stats()["bases_before"] == len(m["bases"])
    got3, m3, pl3 = _same(eng, u, m2, seqs, recs, circular=False, band0=256)            # and a plain round on top: the rounds mix
    assert eng.realign_stats()["round"] == 3 and (pl3["pad"] == 0).all() and eng.realign_stats()["wrapped"] == 0


def test_a_trim_in_force_on_the_circle(eng):
    """circle_plus with 150 junk bases behind read 12: the trim clips them, and the clip is aligned across the origin"""
    seqs, recs = CC.circle_plus(junk=150)
    u = _install(eng, seqs, recs, RC.GRAPH, trim=TRIM)
    assert u["circular"].tolist() == [1] and u["len"].tolist() == [6000]
    clips = eng.graph_clips()
    assert (int(clips["beg"][12]), int(clips["end"][12]), len(seqs[12])) == (0, 800, 950)
    p = _polish(eng, CC.gentle_table(seqs, 3))
    got, m, pl = _same(eng, u, p, seqs, recs, clips=(clips["beg"], clips["end"]), band0=256)
    SEEN["trim"] = pl["status"][12] == R.VOTED and int(pl[12]["q_end"]) > len(p["bases"]) and int(pl[12]["pad"]) == 1


def test_the_cases_cover_what_they_should():
    """over the cases above (pytest keeps file order)"""
    assert all(SEEN.values()), SEEN


# ---- nothing else moves --------------------------------------------------------------------------------------------------------------
def _equal(a, b):
    """two results of _getters: every getter's bytes"""
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert a[4] == b[4], (a[4], b[4])


def test_a_line_through_the_circular_entry_point_is_the_plain_round(eng):
    seqs, recs = RC.line_case()
    u = _install(eng, seqs, recs, RC.GRAPH)
    assert u["circular"].tolist() == [0, 0]
    _polish(eng, RC.line_table(seqs))
    eng.graph_realign_unitigs(keep_ops=1, band0=256)
    plain = _getters(eng)
    _polish(eng, RC.line_table(seqs))
    eng.graph_realign_unitigs(circular=True, keep_ops=1, band0=256)
    _equal(_getters(eng), plain)
    assert plain[4]["wrapped"] == 0 and plain[4]["round"] == 1


def test_a_circle_too_short_for_band_max_and_the_plain_entry_point_keep_their_result(eng):
    seqs, recs = RC.circle_case()
    u = _install(eng, seqs, recs, RC.GRAPH)
    tab = CC.gentle_table(seqs, 3)
    p = _polish(eng, tab)
    got, m, pl = _same(eng, u, p, seqs, recs, circular=False, band0=256)                # the plain entry point: two reads stay outside
    assert (pl["status"] == R.OUTSIDE).sum() == 2 and eng.realign_stats()["outside"] == 2 and (pl["pad"] == 0).all()
    _polish(eng, tab)
    eng.graph_realign_unitigs(keep_ops=1, band0=256, band_max=8192)
    plain = _getters(eng)
    _polish(eng, tab)
    eng.graph_realign_unitigs(circular=True, keep_ops=1, band0=256, band_max=8192)       # 1,500 + 8,192 > 5,993: no read is eligible
    _equal(_getters(eng), plain)
    assert plain[4]["outside"] == 2 and plain[4]["wrapped"] == 0


def test_state_and_errors_of_the_circular_entry_point():
    e = Engine(0)
    try:
        STATE, BAD = -7, -3
        run = lambda **kw: e.graph_realign_unitigs(circular=True, **kw)
        seqs, recs = RC.circle_case()
        e.set_reads(synth.ReadSet.from_strings(seqs))
        e.graph_add_overlaps(recs)
        e.graph_build(**RC.GRAPH)
        e.graph_unitigs()
        e.pileup_reset()
        raises(STATE, run)                                              # before the polish
        raises(STATE, e.realign_stats)
        e.graph_polish_unitigs()
        raises(STATE, e.realign_placements)
        for bad in (dict(band0=300), dict(band0=128), dict(band0=1024, band_max=512), dict(band_max=1 << 19), dict(min_depth=0), dict(min_identity=1001)):
            raises(BAD, lambda: run(**bad))
        with pytest.raises(TypeError):
            run(circle=1)
        small = _lib.RealignParams(C.sizeof(_lib.RealignParams) - 4, 512, 4096, 700, 3, 0)
        assert e.lib.bella_hip_graph_realign_unitigs_circular(e.h, C.byref(small), None) == BAD
        assert e.lib.bella_hip_graph_realign_unitigs_circular(None, None, None) == BAD
        assert e.lib.bella_hip_graph_realign_unitigs_circular(e.h, None, None) == 0         # the defaults; total_bases may be NULL
        assert e.realign_stats()["outside"] == 0 and e.realign_stats()["wrapped"] > 0
        w = C.c_uint64(0)                                                                   # `wrapped` has a getter of its own; the stats struct keeps its size
        assert C.sizeof(_lib.RealignStats) == 176 and e.lib.bella_hip_graph_get_realign_wrapped(e.h, C.byref(w)) == 0 and w.value == e.realign_stats()["wrapped"]
        assert e.lib.bella_hip_graph_get_realign_wrapped(e.h, None) == 0 and e.lib.bella_hip_graph_get_realign_wrapped(None, C.byref(w)) == BAD
        for drop in (lambda: e.graph_cut_weak(), lambda: e.pileup_reset(), lambda: e.graph_polish_unitigs(), lambda: e.graph_unitigs()):
            e.graph_unitigs()
            e.pileup_reset()
            e.graph_polish_unitigs()
            run(band0=256)
            assert e.realign_stats()["round"] == 1
            run(band0=256)
            assert e.realign_stats()["round"] == 2
            drop()
            raises(STATE, e.realign_stats)
            assert e.lib.bella_hip_graph_get_realigned(e.h, None, None, None, None, None) == STATE
            assert e.lib.bella_hip_graph_get_realign_wrapped(e.h, None) == STATE
    finally:
        e.close()


# ---- command line ----------------------------------------------------------------------------------------------------------------
E2E = dict(glen=48000, nreads=240, read_len=8000, err=0.15, seed=0)      # the smallest seed whose pipeline below yields exactly one circular unitig


def _texts(names, u, r):
    q = dict(u)
    q["pos"], q["nbases"], q["len"] = r["pos"], r["nbases"], r["stats"]["len_after"].astype(np.uint64)
    return U.unitig_gfa_text(names, q, r["offsets"], r["bases"]), U.fasta_text(q, r["offsets"], r["bases"])


def _line(round_, st, circular):
    s = "round %d: %d of %d reads realigned (%d unplaced, %d outside, %d band-capped, %d of low identity), " % (
        round_, st["voted"], st["backbone"] + st["contained"] + st["unplaced"], st["unplaced"], st["outside"], st["band_capped"], st["low_identity"])
    return (s + ("%d across an origin, " % st["wrapped"] if circular else "") + "%d -> %d bases" % (st["bases_before"], st["bases_after"])).encode()


def test_cli_realign_circular_end_to_end(eng, tmp_path):
    """240 reads of 8 kb at 15 % error around a circle of 48 kb.  The pipeline of the command line's defaults yields exactly one circular
    unitig (the precondition).  --polish-rounds 2 --realign-circular writes the files Engine gives with circular=True, its log counts the
    reads across an origin and none outside; -m 1 and -g 2 give the same files; without the option the files and the log line are those
    of the plain round."""
    genome, seqs, names = CC.circular_reads(**E2E)
    rs = synth.ReadSet.from_strings(seqs, names)
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    eng.align_pairs(pars)
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    eng.graph_reset()
    eng.graph_add_traced()
    eng.graph_build()
    eng.graph_clean()
    u = eng.graph_unitigs()
    assert u["circular"].tolist() == [1], (u["circular"].tolist(), u["len"].tolist())
    want = {}
    for circular in (False, True):
        eng.graph_polish_unitigs(3)
        r = eng.graph_realign_unitigs(circular=circular)
        want[circular] = _texts(names, u, r) + (_line(2, eng.realign_stats(), circular),)
    st = eng.realign_stats()
    assert st["wrapped"] > 0 and st["outside"] == 0 and want[True][:2] != want[False][:2]
    fq = str(tmp_path / "reads.fastq")
    synth.write_fastq(fq, rs)
    base = ["--unitigs", "u.gfa", "--unitigs-fasta", "u.fa", "--polish", "--polish-rounds", "2"]

    def run(flags, where, env=None):
        f = run_cli([fq], base + flags, str(tmp_path / where), env)
        return (f.get("u.gfa"), f.get("u.fa")), f["stderr"]
    got, err = run(["--realign-circular"], "circ")
    assert got == want[True][:2]
    assert want[True][2] in err and b" 0 outside" in want[True][2] and b"across an origin" in want[True][2]
    print("REALIGN cli:", want[True][2].decode(), "| plain:", want[False][2].decode())
    assert run(["--realign-circular", "-m", "1"], "m1")[0] == want[True][:2]
    assert run(["--realign-circular", "-g", "2"], "g2", {"BELLA_HIP_OVERSUBSCRIBE": "1"})[0] == want[True][:2]
    got, err = run([], "plain")
    assert got == want[False][:2] and want[False][2] in err and b"across an origin" not in err
