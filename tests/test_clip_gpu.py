"""GPU tests of the clipped ends: what k_clip returns EQUALS the numpy mirror (bella_testkit/clip_mirror.py), field
for field, on hand-made pairs at the chunk borders, the tie rules and 64-bit sums (bella_testkit/clip_cases.py) and on random pairs;
through the pipeline the clipped records, the statistics and the pileup tables are the mirror's of the unclipped call; without the
option nothing changes; what the clip buys on reads with junk ends; bella-hip --clip-ends end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib
from bella_testkit import clip_cases as CC
from bella_testkit import clip_mirror as K
from bella_testkit.pipeline import aligned as _aligned, raises, records as _records, run_cli
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu
BAD = -3


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for f in got.dtype.names:
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:8])


def _stats_equal(st, want):
    assert {k: st[k] for k in want} == want, (st, want)
    assert st["clip_ms"] >= 0.0


# ---- clip_ops: the kernel on explicit runs --------------------------------------------------------------------------------------------
def test_hand_made_pairs_at_every_place_the_kernel_can_go_wrong(eng):
    """every case of clip_cases.hand_cases() (tests/test_clip_cpu.py asserts each has the segment it is meant to have), one call per
    identity: CLIP_RES_DT and the statistics equal the mirror's"""
    cases = CC.hand_cases()
    assert tuple(len(c[2]) for c in cases[:len(CC.RUN_COUNTS)]) == CC.RUN_COUNTS
    for t in sorted({c[1] for c in cases}):
        mine = [c for c in cases if c[1] == t]
        pairs, ops = CC.build_batch([c[2] for c in mine], seed=t)
        got = eng.clip_ops(pairs, ops, identity=t)
        want, st = K.clip_pairs(pairs, ops, t)
        _same(got, want)
        _stats_equal(eng.clip_stats(), st)
        for c, r in zip(mine, got):
            if c[3] is not None:
                assert (int(r["first_run"]), int(r["first_run"]) + int(r["nruns"])) == c[3], c[0]
    big = [c for c in cases if c[0] == "2^24 columns"][0]
    r = eng.clip_ops(*CC.build_batch([big[2]]), identity=650)[0]
    assert int(r["clip_score"]) == (1 << 24) * 350 > 2 ** 32 and int(r["n_eq"]) == 1 << 24


@pytest.mark.parametrize("npairs", CC.BATCH_SIZES)
def test_batch_sizes(eng, npairs):
    """1, 3, 4, 5 and 257 pairs: a block holds four wavefronts, so a wavefront alone, a block not full, full, one over and 65 blocks"""
    rng = np.random.default_rng(npairs)
    pairs, ops = CC.build_batch([CC.random_runs(rng, int(rng.integers(0, 140))) for _ in range(npairs)], seed=npairs)
    got = eng.clip_ops(pairs, ops)
    want, st = K.clip_pairs(pairs, ops, 650)
    _same(got, want)
    _stats_equal(eng.clip_stats(), st)


@pytest.fixture(scope="module")
def random_batch():
    return CC.random_batch()


@pytest.mark.parametrize("t", CC.IDENTITIES)
def test_random_pairs(eng, random_batch, t):
    """2,000 random pairs of up to 300 runs"""
    pairs, ops = random_batch
    assert len(pairs) == 2000 and int(pairs["nops"].max()) > 256
    got = eng.clip_ops(pairs, ops, identity=t)
    want, st = K.clip_pairs(pairs, ops, t)
    _same(got, want)
    _stats_equal(eng.clip_stats(), st)
    assert st["identity"] == t == eng.clip_stats()["identity"]


def test_empty_call_and_default_identity(eng):
    pairs, ops = CC.build_batch([CC.good(9), CC.poor(9)])
    out = eng.clip_ops(pairs[:0], ops[:0])
    st = eng.clip_stats()
    assert len(out) == 0 and st["pairs"] == 0 and st["identity"] == 650
    _same(eng.clip_ops(pairs, ops, identity=0), K.clip_pairs(pairs, ops, 650)[0])        # 0: the default
    assert eng.clip_stats()["identity"] == 650
    out = np.zeros(len(pairs), _lib.CLIP_RES_DT)
    assert eng.lib.bella_hip_clip_ops(eng.h, pairs.ctypes.data, len(pairs), ops.ctypes.data, len(ops), None, out.ctypes.data) == 0   # NULL: the default
    _same(out, K.clip_pairs(pairs, ops, 650)[0])


def test_clip_ops_validates_before_it_launches(eng):
    rng = np.random.default_rng(8)
    pairs, ops = CC.build_batch([CC.random_runs(rng, 20), CC.random_runs(rng, 70)])
    good = eng.clip_ops(pairs, ops)
    before = eng.clip_stats()

    def bad(field=None, value=None, op_at=None, op_word=None, cut_ops=0, identity=650):
        p, o = pairs.copy(), ops.copy()
        if field:
            p[field][1] = value
        if op_at is not None:
            o[op_at] = op_word
        o = o[:len(o) - cut_ops]
        out = np.full(len(p), 0xEE, np.uint8).repeat(_lib.CLIP_RES_DT.itemsize).view(_lib.CLIP_RES_DT)
        kp = _lib.ClipParams(C.sizeof(_lib.ClipParams), identity)
        assert eng.lib.bella_hip_clip_ops(eng.h, p.ctypes.data, len(p), o.ctypes.data, len(o), C.byref(kp), out.ctypes.data) == BAD
        assert out.tobytes() == b"\xee" * out.nbytes           # untouched, also the valid first pair's record
        assert eng.clip_stats() == before
    last = int(pairs["op_off"][1]) + int(pairs["nops"][1]) - 1
    bad(op_at=last, op_word=(1 << 4) | 4)                     # an op that is none of = X I D
    bad(op_at=last, op_word=(1 << 4) | 15)
    bad(op_at=last, op_word=0 | 0)                            # a run of length 0
    bad("op_off", len(ops) + 1)                               # op_off past the end
    bad("op_off", len(ops) - 3)                               # op_off + nops past the end
    bad("nops", len(ops))
    bad(cut_ops=2)
    bad("tbegV", -1)
    bad("tbegH", -1)
    bad("tbegV", 2 ** 31 - 10)                                # the pair's last base of V at 2^31 or beyond
    bad(identity=1000)
    bad(identity=4000)
    small = _lib.ClipParams(C.sizeof(_lib.ClipParams) - 4, 650)
    out = np.zeros(len(pairs), _lib.CLIP_RES_DT)
    assert eng.lib.bella_hip_clip_ops(eng.h, pairs.ctypes.data, len(pairs), ops.ctypes.data, len(ops), C.byref(small), out.ctypes.data) == BAD
    assert eng.lib.bella_hip_clip_ops(eng.h, None, 1, None, 0, None, out.ctypes.data) == BAD
    assert eng.lib.bella_hip_clip_ops(eng.h, pairs.ctypes.data, len(pairs), ops.ctypes.data, len(ops), None, None) == BAD
    raises(BAD, eng.clip_ops, pairs, ops, 1000)
    huge = CC.build_batch([[CC.w((1 << 28) - 1, k & 1) for k in range(9)]])               # nine runs of the longest length: V has more than 2^31 bases
    raises(BAD, eng.clip_ops, huge[0], huge[1])
    huge = CC.build_batch([[CC.w((1 << 28) - 1, (CC.DEL, CC.EQ)[k & 1]) for k in range(12)]])   # ... and H alone
    raises(BAD, eng.clip_ops, huge[0], huge[1])
    _same(eng.clip_ops(pairs, ops), good)                     # ... and the context still works
    e2 = Engine(0)                                            # no reads loaded: none are needed
    try:
        _same(e2.clip_ops(pairs, ops), good)
    finally:
        e2.close()


# ---- through the pipeline -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["toy120", "toyjunk220"])
def traced(eng, request):
    """a golden set aligned on the device and its plain traces: (g, pars, pairs, alns, traces, ops)"""
    g = load_golden(request.param)
    pars, pairs, alns = _aligned(eng, g)
    tr, ops = eng.trace_pairs(pars)
    return g, pars, pairs, alns, tr, ops


def _realign(eng, g):
    return _aligned(eng, g)[0]


def test_clipped_records_are_the_mirror_of_the_unclipped_ones(eng, traced):
    g, _, pairs, alns, tr0, ops0 = traced
    pars = _realign(eng, g)
    tr, ops = eng.trace_pairs(pars, clip=650)
    ntraced = int(eng.trace_stats().pairs)
    want, st = K.clip_traces(tr0, ops0, 650)
    assert np.array_equal(ops, ops0)                          # the runs are not rewritten
    _same(tr, want)
    _stats_equal(eng.clip_stats(), st)
    assert st["pairs"] == ntraced == int((tr0["nops"] > 0).sum()) and st["clipped"] > 0
    m = tr["nops"] > 0
    first = tr["op_off"][m].astype(np.int64)
    w0 = ops[first] & 15
    w1 = ops[first + tr["nops"][m].astype(np.int64) - 1] & 15
    assert not w0.any() and not w1.any()                      # every clipped alignment begins and ends with '='
    assert np.array_equal(tr["score"][m], (tr["n_eq"].astype(np.int64) - tr["n_x"] - tr["n_ins"] - tr["n_del"])[m])
    # *ntraced leaves the emptied pairs out; *nops is the call's without the clip
    nt, no = C.c_uint64(0), C.c_uint64(0)
    cp = pars.c()
    kp = _lib.ClipParams(C.sizeof(_lib.ClipParams), 650)
    assert eng.lib.bella_hip_trace_pairs_clip(eng.h, C.byref(cp), 0, _lib.TRACE_PASSED_ONLY, C.byref(kp), C.byref(nt), C.byref(no)) == 0
    assert nt.value == st["pairs"] - st["emptied"] and no.value == len(ops0)
    # the records alone: the same, no run staged
    tr2 = eng.trace_pairs_records(pars, clip=650)
    _same(tr2, want)
    assert eng.trace_stats().ops_host_bytes == 0
    _stats_equal(eng.clip_stats(), st)
    # other identities; 999 empties or shortens nearly everything, 1 keeps nearly everything
    for t in (1, 999):
        tr3, _ = eng.trace_pairs(pars, clip=t)
        want3, st3 = K.clip_traces(tr0, ops0, t)
        _same(tr3, want3)
        _stats_equal(eng.clip_stats(), st3)
    print("CLIP %s at 650: %s" % (g.name, st))


def test_flags_and_parameters_of_the_clipped_trace(eng, traced):
    g = traced[0]
    pars = _realign(eng, g)
    eng.pileup_reset()
    cp = pars.c()
    call = lambda flags, kp: eng.lib.bella_hip_trace_pairs_clip(eng.h, C.byref(cp), 0, flags, kp, None, None)
    ok = C.byref(_lib.ClipParams(C.sizeof(_lib.ClipParams), 650))
    assert call(16, ok) == BAD and call(_lib.TRACE_NORMALIZE, ok) == BAD and call(_lib.TRACE_PILEUP, ok) == BAD
    for t in (1000, 2 ** 31):
        assert call(1, C.byref(_lib.ClipParams(C.sizeof(_lib.ClipParams), t))) == BAD
    assert call(1, C.byref(_lib.ClipParams(4, 650))) == BAD
    assert int(eng.get_pileup().sum(dtype=np.int64)) == 0
    assert call(1, None) == 0 and eng.clip_stats()["identity"] == 650
    assert call(1, C.byref(_lib.ClipParams(C.sizeof(_lib.ClipParams), 0))) == 0 and eng.clip_stats()["identity"] == 650
    raises(BAD, eng.trace_pairs, pars, clip=1000)
    with pytest.raises(ValueError):
        eng.trace_pairs(pars, normalize=True, clip=650)


@pytest.mark.parametrize("normalize", [False, True])
def test_pileup_of_clipped_pairs(eng, traced, normalize):
    """trace_pairs(pileup=True, clip=650): the table is the one pileup_vote builds from the clipped records and the same runs; with
    keep_ops=False records and table are the same"""
    g, _, pairs, alns, tr0, ops0 = traced
    pars = _realign(eng, g)
    want, st = K.clip_traces(tr0, ops0, 650)
    eng.pileup_reset()
    tr, ops = eng.trace_pairs(pars, pileup=True, normalize=normalize, clip=650)
    table = eng.get_pileup()
    vs = eng.vote_stats()
    _same(tr, want)
    assert np.array_equal(ops, ops0)
    _stats_equal(eng.clip_stats(), st)
    eng.pileup_reset()
    tr2, ops2 = eng.trace_pairs(pars, pileup=True, normalize=normalize, keep_ops=False, clip=650)
    assert len(ops2) == 0 and tr2.tobytes() == tr.tobytes() and np.array_equal(eng.get_pileup(), table)
    _stats_equal(eng.clip_stats(), st)
    eng.pileup_reset()
    eng.pileup_vote(K.vote_pairs(pairs, alns, want), ops0, normalize=normalize)
    assert np.array_equal(eng.get_pileup(), table)
    vs2 = eng.vote_stats()
    assert vs["pairs"] == vs2["pairs"] == st["pairs"] - st["emptied"] and vs["runs"] == vs2["runs"] == st["runs_after"] and vs["votes"] == vs2["votes"]
    # the clip changed the votes: the unclipped table is another one
    eng.pileup_reset()
    eng.pileup_vote(K.vote_pairs(pairs, alns, tr0), ops0, normalize=normalize)
    assert not np.array_equal(eng.get_pileup(), table)


def test_graph_records_after_a_clipped_trace(eng, traced):
    g, _, pairs, alns, tr0, ops0 = traced
    pars = _realign(eng, g)
    want, _ = K.clip_traces(tr0, ops0, 650)
    for records_only in (False, True):
        if records_only:
            eng.trace_pairs_records(pars, clip=650)
        else:
            eng.trace_pairs(pars, clip=650)
        eng.graph_reset()
        n = eng.graph_add_traced()
        got = eng.graph_overlaps()
        recs = _records(pairs, alns, want)
        assert n == len(recs) == int(((alns["passed"] == 1) & (want["nops"] > 0)).sum())
        assert got.tobytes() == recs.tobytes()
    plain = _records(pairs, alns, tr0)
    assert len(plain) >= len(recs) and plain.tobytes() != recs.tobytes()


def test_without_clip_nothing_changes(eng, traced):
    """the calls of today after clipped ones: records, runs and tables are those of a plain call made before any clip"""
    g, _, pairs, alns, tr0, ops0 = traced
    pars = _realign(eng, g)
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, clip=650)
    tr, ops = eng.trace_pairs(pars)
    assert tr.tobytes() == tr0.tobytes() and ops.tobytes() == ops0.tobytes()
    assert eng.trace_pairs_records(pars).tobytes() == tr0.tobytes()
    tables = []
    for _ in range(2):
        eng.pileup_reset()
        tr, ops = eng.trace_pairs(pars, pileup=True)
        assert tr.tobytes() == tr0.tobytes() and ops.tobytes() == ops0.tobytes()
        tables.append(eng.get_pileup())
    eng.pileup_reset()
    eng.pileup_vote(K.vote_pairs(pairs, alns, tr0), ops0)
    assert np.array_equal(tables[0], tables[1]) and np.array_equal(tables[0], eng.get_pileup())


# ---- what it buys ---------------------------------------------------------------------------------------------------------------------
def test_clipped_ends_bring_the_trim_to_the_true_boundaries(eng):
    """300 synthetic reads of about 5 kb at 15 % error, 30x; 600 to 1,500 random bases on 40 % of the ends, head and tail known.  count ->
    overlap -> align -> trace -> graph_add_traced -> graph_trim, with and without clip=650.  Conditions: with the clip the summed
    distance of the trim's clips to the true boundaries over the junk reads is strictly smaller, and so is bases_after.  The sums and
    the median distance per read are printed, not asserted (DESIGN.md section 24 has them).
    Measured on an MI355X: 203 junk reads with 285,737 junk bases; summed distance 275,429 without and 130,739 with the clip, median per
    read 1,221 and 500 (the trim's own end_clip); bases_after 1,840,775 and 1,435,496 of 1,853,133; 4,446 of 6,710 pairs clipped."""
    rs, head, tail, lens = CC.junk_reads()
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    assert eng.align_pairs(pars) > 300
    junk = np.flatnonzero((head > 0) | (tail > 0))
    assert len(junk) > 100
    res = {}
    for clip in (None, 650):
        eng.trace_pairs_records(pars, clip=clip)
        ts = eng.trace_stats()
        ks = eng.clip_stats() if clip else None
        eng.graph_reset()
        eng.graph_add_traced()
        eng.graph_trim()
        c = eng.graph_clips()
        st = eng.trim_stats()
        covered = junk[c["end"][junk] > c["beg"][junk]]
        d = np.abs(c["beg"][covered].astype(np.int64) - head[covered]) + np.abs(c["end"][covered].astype(np.int64) - (head[covered] + lens[covered]))
        # (a junk read the trim leaves uncovered counts with its whole true span)
        lost = np.setdiff1d(junk, covered)
        res[clip] = dict(dist=int(d.sum()) + int(lens[lost].sum()), median=float(np.median(d)) if len(d) else -1.0, uncovered=len(lost),
                         bases_before=st["bases_before"], bases_after=st["bases_after"], walk_ms=ts.walk_ms, clip_ms=ks["clip_ms"] if ks else 0.0,
                         clipped=ks["clipped"] if ks else 0, emptied=ks["emptied"] if ks else 0, pairs=int(ts.pairs))
    junk_bases = int(head.sum() + tail.sum())
    print("CLIP effect: %d reads, %d with junk, %d junk bases, %d true bases; without / with clip=650: %s / %s"
          % (rs.nreads, len(junk), junk_bases, int(lens.sum()), res[None], res[650]))
    assert res[650]["dist"] < res[None]["dist"], res
    assert res[650]["bases_after"] < res[None]["bases_after"], res


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_clip_ends_end_to_end(eng, tmp_path):
    """bella-hip --gfa --trim --clip-ends on toyjunk220: runs; the -o file is byte for byte the one without the option; the log's
    ClippedEnds line carries the Python path's sums; -m 1 gives the same GFA; the GFA differs from the one without the option"""
    g = load_golden("toyjunk220")
    pars, pairs, alns = _aligned(eng, g)
    eng.trace_pairs_records(pars, clip=650)
    ks = eng.clip_stats()
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r + 1, k + 1, q) for k, r, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    base = g.meta["flags"] + ["--tuples", mtx, "--gfa", "g.gfa", "--gfa-min-overlap", "0", "--gfa-fuzz", "10", "--trim", "--trim-depth", "2", "--trim-end-clip", "20"]
    plain = run_cli([fq], base, str(tmp_path / "plain"))
    assert plain["out.out"] == g.out["align"] and b"ClippedEnds" not in plain["stderr"]
    files = run_cli([fq], base + ["--clip-ends"], str(tmp_path / "clip"))
    assert files["out.out"] == g.out["align"]
    log = [ln for ln in files["stderr"].decode().splitlines() if "ClippedEnds = " in ln]
    assert len(log) == 1
    want = "%d clipped, %d emptied (of %d traced pairs at identity 650), %d of %d columns removed, %d bases" % (
        ks["clipped"], ks["emptied"], ks["pairs"], ks["columns_before"] - ks["columns_after"], ks["columns_before"], ks["bases_v_removed"] + ks["bases_h_removed"])
    assert want in log[0], (want, log[0])
    assert files["g.gfa"] != plain["g.gfa"]
    m1 = run_cli([fq], base + ["--clip-ends", "--clip-identity", "650", "-m", "1"], str(tmp_path / "m1"))
    assert m1["g.gfa"] == files["g.gfa"] and m1["out.out"] == g.out["align"]
    assert want in [ln for ln in m1["stderr"].decode().splitlines() if "ClippedEnds = " in ln][0]
    print("CLIP cli toyjunk220: %s" % log[0].split("ClippedEnds = ")[1])
