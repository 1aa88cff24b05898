"""GPU tests of the link alignment: the device result EQUALS the mirror (bella_testkit/links_mirror.py) on every
field of every link and on the runs, on the layouts of bella_testkit/link_cases.py -- raw, polished and after a realignment round; the
same call in one link per batch (BELLA_TUNE_ROUND_BUDGET); state and errors; and the command line, whose L lines are replayed on the
file's own S lines."""
import ctypes as C
import re

import numpy as np
import pytest

from bella_amd import Engine, _lib
from bella_testkit import link_cases as LC
from bella_testkit import links_mirror as LM
from bella_testkit import synth
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import raises, run_cli, with_round_budget

pytestmark = pytest.mark.gpu

SEEN = dict(plus_plus=False, plus_minus=False, minus_plus=False, minus_minus=False, m_is_the_unitig=False, n_is_the_unitig=False, doubled=False, capped=False, wide=False, dp16=False,
            aligned=False, empty=False, band_capped=False, low_identity=False, self_link=False, derived=False, polished=False, realigned=False)
SIGNS = {0: "plus_plus", LM.B_MINUS: "plus_minus", LM.A_MINUS: "minus_plus", LM.A_MINUS | LM.B_MINUS: "minus_minus"}
STATUS = {LM.ALIGNED: "aligned", LM.EMPTY: "empty", LM.BAND_CAPPED: "band_capped", LM.LOW_IDENTITY: "low_identity", LM.SELF: "self_link"}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _install(eng, seqs, recs):
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_reset()
    eng.graph_add_overlaps(recs)
    eng.graph_build(**LC.GRAPH)
    eng.graph_clean(**LC.CLEAN)
    u = eng.graph_unitigs()
    u["offsets"], u["bases"] = eng.unitig_bases()
    return u


def _polish(eng, table):
    eng.pileup_reset()
    eng.add_pileup(0, eng.nreads, table)
    return eng.graph_polish_unitigs(3)


def _getters(eng, **params):
    n = eng.graph_align_links(**params)
    alns, ops = eng.link_alignments()
    return dict(n=np.array([n]), alns=alns, ops=ops, st=eng.link_stats())


def _same(eng, u, cur=None, **params):
    """one call on the device against the mirror's on `cur` (None: the raw unitigs): every field of every link, the runs, the counts"""
    got = _getters(eng, **params)
    m = LM.align_links(u, cur, **{**LM.DEFAULTS, **params})
    alns, ops = got["alns"], got["ops"]
    assert alns.dtype == _lib.LINK_ALN_DT == LM.ALN_DT and ops.dtype == np.uint32
    for f in LM.ALN_DT.names:
        assert np.array_equal(alns[f], m["alns"][f]), (f, alns[f], m["alns"][f])
    assert np.array_equal(ops, m["ops"])
    st = got["st"]
    assert {k: st[k] for k in m["counts"]} == m["counts"]
    assert int(got["n"][0]) == m["counts"]["aligned"]
    band_max = params.get("band_max", LM.DEFAULTS["band_max"])
    coffs = (cur["offsets"] if cur is not None else u["offsets"]).astype(np.int64)
    for k, (l, a) in enumerate(zip(u["links"], alns)):
        SEEN[STATUS[int(a["status"])]] = True
        SEEN["derived"] |= bool(a["derived"])
        if int(a["status"]) == LM.SELF or int(a["derived"]):
            continue
        SEEN[SIGNS[int(l["flags"]) & 3]] = True                        # of the links the device aligned
        w = LM.windows(u, cur, k, band_max)
        SEEN["m_is_the_unitig"] |= w["m"] == int(coffs[int(l["a"]) + 1] - coffs[int(l["a"])]) < w["oa"] + band_max // 2
        SEEN["n_is_the_unitig"] |= w["n"] == int(coffs[int(l["b"]) + 1] - coffs[int(l["b"])]) < w["ob"] + band_max // 2
        if int(a["status"]) == LM.ALIGNED:                             # and what it found is an alignment of the two windows
            got_counts = LM.replay(ops[int(a["op_off"]):int(a["op_off"]) + int(a["nops"])], w["X"], w["Y"], int(a["ovl_a"]), int(a["ovl_b"]))
            assert got_counts["score"] == int(a["score"])
    return got, m


# ---- 1. the fork ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", ["", "b", "ta"])
def test_the_fork_raw_equals_the_mirror(eng, rev):
    """three unitigs, four links; the numbering of the reads chooses the links' signs: + +, + - and, with the trunk against the line,
    - - and - +"""
    seqs, recs, _ = LC.fork_case(rev=rev)
    u = _install(eng, seqs, recs)
    assert sorted(u["len"].tolist()) == [4400, 5600, 5600] and len(u["links"]) == 4
    got, m = _same(eng, u)
    st = got["st"]
    assert st["jobs"] == 2 and st["derived"] == 2 and st["aligned"] == 4 and st["batches"] == 1
    assert got["alns"]["ovl_a"].tolist() == [800] * 4 and got["alns"]["n_eq"].tolist() == [800] * 4
    print("LINKS fork raw %r: %s; pack %.3f ms, dp %.3f ms, walk %.3f ms" % (rev, m["counts"], st["pack_ms"], st["dp_ms"], st["walk_ms"]))


def test_the_fork_polished_equals_the_mirror(eng):
    """polished with fork_table: the trunk loses every 97th base, the arms gain one before every 61st, so oa != ob and the alignments
    have gaps"""
    seqs, recs, trunk = LC.fork_case(rev="b")
    u = _install(eng, seqs, recs)
    p = _polish(eng, LC.fork_table(seqs, trunk))
    assert len(p["bases"]) != int(u["len"].sum())
    got, m = _same(eng, u, p)
    w = LM.windows(u, p, 0, 4096)
    assert w["oa"] != w["ob"] and m["counts"]["aligned"] == 4
    assert (got["alns"]["n_ins"] + got["alns"]["n_del"] > 0).all()
    SEEN["polished"] = True
    print("LINKS fork polished: %s, overlaps %s -> %s" % (m["counts"], m["expected"].tolist(), got["alns"]["ovl_a"].tolist()))


def test_the_fork_after_a_realignment_round_equals_the_mirror(eng):
    seqs, recs, trunk = LC.fork_case(rev="ta")
    u = _install(eng, seqs, recs)
    _polish(eng, LC.fork_table(seqs, trunk))
    r = eng.graph_realign_unitigs()
    got, m = _same(eng, u, r)
    assert m["counts"]["aligned"] == 4
    SEEN["realigned"] = True


# ---- 2. a one-read arm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["tab", "bat"])
def test_a_one_read_arm(eng, order):
    """arm b is one read of 2,000 bases.  Numbered last, the aligned link enters it: n = P_b; numbered first, the aligned link leaves it:
    m = P_a"""
    seqs, recs, _ = LC.fork_case(arms=(4, 1), order=order)
    u = _install(eng, seqs, recs)
    assert sorted(u["len"].tolist()) == [2000, 4400, 5600]
    _same(eng, u)
    assert SEEN["n_is_the_unitig" if order == "tab" else "m_is_the_unitig"]


# ---- 3. - 5. the bands ---------------------------------------------------------------------------------------------------------------
def test_a_deletion_of_120_bases_doubles_the_band(eng):
    seqs, recs, _ = LC.fork_case(deleted=120)
    u = _install(eng, seqs, recs)
    got, m = _same(eng, u, band0=256)
    alns = got["alns"]
    assert sorted(alns["band"].tolist()) == [256, 256, 512, 512] and (alns["status"] == LM.ALIGNED).all()
    k = int(np.flatnonzero((alns["band"] == 512) & (alns["derived"] == 0))[0])
    assert (int(alns[k]["n_del"]), int(alns[k]["n_eq"]), int(alns[k]["ovl_a"]), int(alns[k]["ovl_b"])) == (120, 680, 800, 680)
    assert got["st"]["batches"] == 2
    SEEN["doubled"] = True


def test_a_deletion_of_248_bases_is_band_capped_at_512(eng):
    seqs, recs, _ = LC.fork_case(deleted=248)
    u = _install(eng, seqs, recs)
    got, m = _same(eng, u, band0=512, band_max=512)
    assert sorted(got["alns"]["status"].tolist()) == [LM.ALIGNED, LM.ALIGNED, LM.BAND_CAPPED, LM.BAND_CAPPED]
    assert (got["alns"]["nops"][got["alns"]["status"] == LM.BAND_CAPPED] == 0).all()
    SEEN["capped"] = True


def test_the_wide_kernel(eng):
    """band0 = 2,048 on the polished fork: every DP runs in the wide kernel"""
    seqs, recs, trunk = LC.fork_case(rev="b")
    u = _install(eng, seqs, recs)
    p = _polish(eng, LC.fork_table(seqs, trunk))
    got, m = _same(eng, u, p, band0=2048)
    assert (got["alns"]["band"] == 2048).all() and m["counts"]["aligned"] == 4
    SEEN["wide"] = True


def test_the_register_kernel_of_16_cells_a_lane(eng):
    """band0 = 1,024 on the polished fork (rev="b", the wide kernel's case): every DP runs in k_lnk_dp<16>, which bands of 256, 512 and
    2,048 never reach.  The mirror aligns all four links at this band (checked on the CPU before the test was written)"""
    seqs, recs, trunk = LC.fork_case(rev="b")
    u = _install(eng, seqs, recs)
    p = _polish(eng, LC.fork_table(seqs, trunk))
    got, m = _same(eng, u, p, band0=1024)
    assert (got["alns"]["band"] == 1024).all() and (got["alns"]["status"] == LM.ALIGNED).all() and len(got["alns"]) == 4
    assert m["counts"]["aligned"] == 4
    SEEN["dp16"] = True


# ---- 6. 7. links that are no overlaps -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forged", [True, "A"])
def test_a_forged_record_between_unrelated_reads(eng, forged):
    """a read of random bases: an alignment of low identity; a read of 2,000 times A: no path scores above 0"""
    seqs, recs, _ = LC.fork_case(forged=forged)
    u = _install(eng, seqs, recs)
    assert len(u["links"]) == 6
    got, m = _same(eng, u)
    bad = LM.LOW_IDENTITY if forged is True else LM.EMPTY
    assert sorted(got["alns"]["status"].tolist()) == sorted([LM.ALIGNED] * 4 + [bad] * 2)
    assert got["st"]["ops"] == int(got["alns"]["nops"].sum()) and (got["alns"]["nops"][got["alns"]["status"] == bad] == 0).all()


def test_a_link_of_a_unitig_to_itself_is_never_aligned(eng):
    seqs, recs = LC.self_case()
    u = _install(eng, seqs, recs)
    is_self = u["links"]["a"] == u["links"]["b"]
    assert is_self.sum() == 2 and len(u["links"]) == 4
    got, m = _same(eng, u)
    assert (got["alns"]["status"][is_self] == LM.SELF).all() and (got["alns"]["band"][is_self] == 0).all() and (got["alns"]["mate"][is_self] == LM.NO).all()
    assert got["st"]["self"] == 2 and got["st"]["jobs"] == 1 and got["st"]["batches"] == 1          # the one DP is the other pair's


# ---- 8. one link per batch -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [dict(), dict(band0=256)])
def test_one_link_per_batch_gives_the_same_result(eng, params):
    """round_budget = 1: every batch takes exactly one link, so dir_off, op_off and the pending list carry over after every link -- on
    the polished fork, and on the fork whose deletion doubles the band"""
    seqs, recs, trunk = LC.fork_case(rev="b") if not params else LC.fork_case(deleted=120)
    _install(eng, seqs, recs)
    if not params:
        _polish(eng, LC.fork_table(seqs, trunk))
    one = _getters(eng, **params)
    many = with_round_budget(eng, 1, lambda: _getters(eng, **params))
    for k in ("n", "alns", "ops"):
        assert one[k].dtype == many[k].dtype and one[k].tobytes() == many[k].tobytes(), k
    skip = ("batches", "pack_ms", "dp_ms", "walk_ms")
    assert {f: v for f, v in one["st"].items() if f not in skip} == {f: v for f, v in many["st"].items() if f not in skip}
    dps = int((np.log2(one["alns"]["band"][one["alns"]["derived"] == 0] // params.get("band0", 512)).astype(np.int64) + 1).sum())
    assert many["st"]["batches"] == dps > one["st"]["batches"]


def test_the_cases_cover_what_they_should():
    """over the cases above (pytest keeps file order): every sign combination among the links the device aligned, both window clamps, a
    doubled band, a capped link, the wide kernel, the widest register kernel, every status, derived twins, a polished and a realigned sequence"""
    assert all(SEEN.values()), SEEN


# ---- state and errors ------------------------------------------------------------------------------------------------------------------
def test_zero_links_launch_nothing(eng):
    seqs, recs, _ = LC.fork_case(arms=(4,))
    u = _install(eng, seqs, recs)
    assert len(u["links"]) == 0 and len(u["len"]) == 1
    assert eng.graph_align_links() == 0
    alns, ops = eng.link_alignments()
    st = eng.link_stats()
    assert len(alns) == 0 and len(ops) == 0 and st["batches"] == 0 and st["jobs"] == 0 and st["dp_ms"] == 0 and st["pack_ms"] == 0


def test_state_and_errors():
    e = Engine(0)
    try:
        STATE, BAD = -7, -3
        seqs, recs, trunk = LC.fork_case()
        e.set_reads(synth.ReadSet.from_strings(seqs))
        e.graph_add_overlaps(recs)
        e.graph_build(**LC.GRAPH)
        raises(STATE, e.graph_align_links)                              # before the unitigs
        raises(STATE, e.link_stats)
        e.graph_clean(**LC.CLEAN)
        e.graph_unitigs()
        raises(STATE, e.link_alignments)
        for bad in (dict(band0=300), dict(band0=128), dict(band0=1024, band_max=512), dict(band_max=8192), dict(min_identity=1001)):
            raises(BAD, lambda: e.graph_align_links(**bad))
        raises(STATE, e.link_stats)
        small = _lib.LinkParams(C.sizeof(_lib.LinkParams) - 4, 512, 4096, 700)
        assert e.lib.bella_hip_graph_align_links(e.h, C.byref(small), None) == BAD

        class Longer(C.Structure):                                      # a later header's struct: eight more bytes, all zero
            _fields_ = _lib.LinkParams._fields_ + [("more", C.c_uint64)]
        longer = Longer(C.sizeof(Longer), 512, 4096, 700, 0)
        assert e.lib.bella_hip_graph_align_links(e.h, C.cast(C.byref(longer), C.POINTER(_lib.LinkParams)), None) == 0
        assert e.lib.bella_hip_graph_align_links(e.h, None, None) == 0                      # the defaults; naligned may be NULL
        assert e.lib.bella_hip_graph_get_link_alignments(e.h, None, None, None) == 0
        buf = (C.c_uint8 * 16)(*([0xEE] * 16))                          # a caller with an older, shorter stats struct: only its bytes are written
        assert e.lib.bella_hip_graph_get_link_stats(e.h, buf, 8) == 0
        assert bytes(buf[:8]) == (4).to_bytes(8, "little") and bytes(buf[8:]) == b"\xee" * 8
        raw = e.link_alignments()[0]

        def polish():
            e.pileup_reset()
            e.add_pileup(0, e.nreads, LC.fork_table(seqs, trunk))
            e.graph_polish_unitigs()
        polish()
        raises(STATE, e.link_stats)                                     # dropped by the polish
        e.graph_align_links()
        assert not np.array_equal(e.link_alignments()[0]["ovl_a"], raw["ovl_a"])             # aligned on the polished sequences
        e.graph_realign_unitigs()
        raises(STATE, e.link_stats)                                     # ... by a realignment round
        e.graph_align_links()
        e.graph_realign_unitigs()
        raises(STATE, e.link_alignments)                                # ... and by the next one
        e.graph_align_links()
        assert e.realign_stats()["round"] == 2 and e.polish_stats()["unitigs"] == 3          # the other getters are as they were
        e.graph_unitigs()
        raises(STATE, e.link_stats)                                     # ... by new unitigs
        e.graph_align_links()
        e.set_reads(synth.ReadSet.from_strings(seqs))
        raises(STATE, e.link_stats)                                     # ... and by new reads
    finally:
        e.close()


# ---- command line -------------------------------------------------------------------------------------------------------------------
L_TODAY = re.compile(rb"^L\tutg\d{6}[lc]\t[+-]\tutg\d{6}[lc]\t[+-]\t\d+M\trc:i:\d+$")
L_ALIGNED = re.compile(rb"^L\t(utg\d{6}[lc])\t([+-])\t(utg\d{6}[lc])\t([+-])\t((?:\d+[MID])+)\trc:i:(\d+)\tNM:i:(\d+)\tol:i:(\d+)$")


def _gfa(text):
    """-> (S sequences by name, L lines)"""
    seq, links = {}, []
    for ln in text.split(b"\n"):
        f = ln.split(b"\t")
        if f[0] == b"S":
            seq[f[1]] = f[2]
        elif f[0] == b"L":
            links.append(ln)
    return seq, links


def _replay_cigar(cigar, A, B):
    """the CIGAR on the oriented sequences: -> (columns that are no match, bases of A's suffix, bases of B's prefix)"""
    runs = [(int(n), op) for n, op in re.findall(rb"(\d+)([MID])", cigar)]
    la = sum(n for n, op in runs if op in b"MD")
    q, i, nm = len(A) - la, 0, 0
    assert q >= 0
    for n, op in runs:
        if op == b"M":
            nm += sum(1 for t in range(n) if A[q + t] != B[i + t])
            q, i = q + n, i + n
        elif op == b"I":
            i, nm = i + n, nm + n
        else:
            q, nm = q + n, nm + n
    assert q == len(A) and i <= len(B)
    return nm, la, i


def _check_links(text, want_aligned):
    seq, links = _gfa(text)
    parsed = {}
    for ln in links:
        m = L_ALIGNED.match(ln)
        if not m:
            assert L_TODAY.match(ln), ln
            continue
        a, sa, b, sb, cigar, rec, nm, ol = m.groups()
        A = U.revcomp(seq[a]) if sa == b"-" else seq[a]
        B = U.revcomp(seq[b]) if sb == b"-" else seq[b]
        got_nm, la, lb = _replay_cigar(cigar, A, B)
        assert got_nm == int(nm), ln
        parsed[(a, sa, b, sb, rec)] = re.findall(rb"(\d+)([MID])", cigar)
    assert len(parsed) == want_aligned
    flip = {b"+": b"-", b"-": b"+"}
    swap = {b"M": b"M", b"I": b"D", b"D": b"I"}
    for (a, sa, b, sb, rec), runs in parsed.items():                   # a twin's line is the reversal of its mate's
        assert parsed[(b, flip[sb], a, flip[sa], rec)] == [(n, swap[op]) for n, op in runs[::-1]]
    return links


def test_cli_align_links_end_to_end(tmp_path):
    """bella-hip --unitigs on a fork written as FASTQ (exact reads in the trunk, 3 % errors in the arms).  Without --align-links every L line is <ovl>M rc:i:, the parent's format; with it
    every ALIGNED line's CIGAR replays on the file's own S lines with exactly NM columns that are no match, and a twin's line is the
    reversal of its mate's -- on the raw unitigs and after --polish --polish-rounds 2; --gfa-no-seq changes no L line; -m 2 and -g 2 give
    the same file; the bad combinations are refused"""
    seqs, _, _ = LC.fork_case(rev="b", trunk_len=4400, gap=1600, noise=0.03)     # (link_cases.py says why the pipeline's fork is this one)
    fq = str(tmp_path / "fork.fastq")
    with open(fq, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b"@r%02d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)))
    base = ["--gfa-min-overlap", "200", "--gfa-fuzz", "10", "--tip-reads", "0", "--unitigs", "u.gfa"]
    plain = run_cli([fq], base, str(tmp_path / "plain"))
    seq0, links0 = _gfa(plain["u.gfa"])
    assert len(seq0) == 3 and len(links0) == 4 and all(L_TODAY.match(ln) for ln in links0) and b"AlignedLinks" not in plain["stderr"]
    al = run_cli([fq], base + ["--align-links"], str(tmp_path / "al"))
    assert al["out.out"] == plain["out.out"]
    assert al["u.gfa"][:al["u.gfa"].index(b"L\t")] == plain["u.gfa"][:plain["u.gfa"].index(b"L\t")]
    links = _check_links(al["u.gfa"], 4)
    assert all(int(L_ALIGNED.match(ln).group(7)) > 0 for ln in links)                     # the arms' reads have errors: no link is <n>M, NM:i:0
    assert [ln.split(b"\t")[:5] for ln in links] == [ln.split(b"\t")[:5] for ln in links0]
    assert b"AlignedLinks = 4 of 4 links aligned (0 empty, 0 band-capped, 0 of low identity, 0 self), 2 derived from their twins, " in al["stderr"]
    assert run_cli([fq], base + ["--align-links", "-m", "2"], str(tmp_path / "m2"))["u.gfa"] == al["u.gfa"]
    assert run_cli([fq], base + ["--align-links", "-g", "2"], str(tmp_path / "g2"), {"BELLA_HIP_OVERSUBSCRIBE": "1"})["u.gfa"] == al["u.gfa"]
    noseq = run_cli([fq], base + ["--align-links", "--gfa-no-seq", "--link-band", "256", "--link-min-identity", "600"], str(tmp_path / "noseq"))
    assert _gfa(noseq["u.gfa"])[1] == links
    pol = run_cli([fq], base + ["--polish", "--polish-rounds", "2", "--align-links"], str(tmp_path / "pol"))
    _check_links(pol["u.gfa"], 4)
    assert b"Realigned = round 2" in pol["stderr"] and b"AlignedLinks = 4 of 4" in pol["stderr"]
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bella_amd", "bin", "bella-hip")
    for bad, msg in ((["--align-links"], b"--align-links needs --unitigs"), (["--unitigs", "u.gfa", "--link-band", "512"], b"need --align-links"),
                     (["--unitigs", "u.gfa", "--align-links", "--link-band", "300"], b"--link-band must be a power of two"),
                     (["--unitigs", "u.gfa", "--align-links", "--link-min-identity", "1001"], b"--link-min-identity")):
        p = subprocess.run([exe, "-f", "in.txt", "-o", "x"] + bad, cwd=str(tmp_path / "plain"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and msg in p.stderr, (bad, p.stderr)
