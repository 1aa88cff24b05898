"""CPU tests of the link alignment's definition (bella_testkit/links_mirror.py): the banded dovetail DP against a
plain full-matrix one, the window and centre arithmetic by hand, the pairing of twins and the derivation of a twin's runs, and the text
of the L lines -- api.link_cigars, the library's writer (plain host code) and its unchanged default."""
import numpy as np
import pytest

from bella_amd import _lib, api
from bella_testkit import link_cases as LC
from bella_testkit import links_mirror as LM
from bella_testkit import realign_mirror as R
from bella_testkit import unitig_mirror as U


def _planted(rng, i):
    """a pair of 50 .. 300 bases with a planted overlap: a suffix of x and a prefix of y come from one template, with errors"""
    m, n = (int(v) for v in rng.integers(50, 301, 2))
    ovl = int(rng.integers(10, min(m, n) + 1))
    t = U.random_genome(ovl, 1000 + i)
    noisy = lambda s: b"".join(bytes([b]) if rng.random() > 0.1 else (b"" if rng.random() < 0.3 else bytes([b"ACGT"[int(rng.integers(0, 4))]]) + (bytes([b]) if rng.random() < 0.4 else b""))
                               for b in s)
    x = (U.random_genome(m - ovl, 2000 + i) + noisy(t))[-m:]
    y = (noisy(t) + U.random_genome(n - ovl, 3000 + i))[:n]
    return x, y


def test_the_banded_dovetail_equals_the_full_matrix():
    """240 random pairs with planted overlaps, a band wide enough to hold the whole matrix whatever the centre: score, i_end and q_begin
    equal the plain DP's under the stated tie rules; the ops replay and their counts give the score"""
    rng = np.random.default_rng(26)
    for i in range(240):
        x, y = _planted(rng, i)
        m, n = len(x), len(y)
        c = int(rng.integers(-20, m + 1))                              # any centre: the band covers -n .. m around it
        res = LM.dovetail_banded(x, y, c, 2048)
        want = LM.dovetail_full(x, y)
        assert (res["score"], res["i_end"], res["q_begin"]) == want, (i, want)
        assert not res["touch"]
        runs = LM.run_lengths(res["ops"])
        got = LM.replay(runs, x, y, m - res["q_begin"], res["i_end"])
        assert got["score"] == res["score"]
    x = U.random_genome(80, 1)
    assert LM.dovetail_full(x, b"") == (0, 0, 80) and LM.dovetail_banded(x, b"", 80, 256)["ops"] == []
    # unrelated sequences of one letter each: nothing scores, the end stays in row 0
    assert LM.dovetail_full(b"A" * 60, b"C" * 60) == (0, 0, 60)
    res = LM.dovetail_banded(b"A" * 60, b"C" * 60, 30, 256)
    assert (res["score"], res["i_end"], res["q_begin"], res["ops"]) == (0, 0, 60, [])


def test_ties_in_the_last_column_go_to_the_smallest_row():
    """x = ACAC, y = ACTTAC.  Column 4: row 2 holds 2 (y's AC on x's last AC), row 6 holds 2 as well (AC on AC, TT inserted, AC on AC:
    2 - 2 + 2), no row holds more: the end is row 2, and the walk from it begins at column 2"""
    x, y = b"ACAC", b"ACTTAC"
    assert LM.dovetail_full(x, y) == (2, 2, 2)
    res = LM.dovetail_banded(x, y, 1, 256)
    assert (res["score"], res["i_end"], res["q_begin"], res["ops"]) == (2, 2, 2, [0, 0])


def _hand():
    """three unitigs: 0 of 5,000 raw bases in two segments, 1 % shorter now; 1 of 3,000 bases, 2 % longer now; 2 of 1,000, unchanged"""
    u = dict(voff=np.array([0, 2, 3, 4], np.uint64), pos=np.array([0, 3000, 0, 0], np.uint64), nbases=np.array([3000, 2000, 3000, 1000], np.uint32),
             len=np.array([5000, 3000, 1000], np.uint64), circular=np.zeros(3, np.uint8))
    bases = U.random_genome(4950 + 3060 + 1000, 7)
    cur = dict(offsets=np.array([0, 4950, 8010, 9010], np.uint64), bases=bases, pos=np.array([0, 2970, 0, 0], np.uint64), nbases=np.array([2970, 1980, 3060, 1000], np.uint32))
    return u, cur, (bases[:4950], bases[4950:8010], bases[8010:])


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_windows_and_centre_by_hand(flags):
    """ovl = 800, band_max = 1024 (S = 512), unitig 0 -> unitig 1 under the four sign combinations.
    A plus:  oa = P_a - C_a(5000 - 800) = 4950 - (2970 + 1200 * 1980 // 2000) = 4950 - 4158 = 792;  A minus: oa = C_a(800) = 800 * 2970 // 3000 = 792
    B plus:  ob = C_b(800) = 800 * 3060 // 3000 = 816;  B minus: ob = P_b - C_b(2200) = 3060 - 2244 = 816
    m = min(4950, 792 + 512) = 1304, n = min(3060, 816 + 512) = 1328, c = 1304 - (792 + 816) // 2 = 500"""
    u, cur, (s0, s1, _) = _hand()
    u["links"] = np.array([(0, 1, 800, 5, flags, 0)], U.LINK_DT)
    w = LM.windows(u, cur, 0, 1024)
    assert (w["oa"], w["ob"], w["m"], w["n"], w["c"]) == (792, 816, 1304, 1328, 500)
    A = U.revcomp(s0) if flags & 1 else s0
    B = U.revcomp(s1) if flags & 2 else s1
    assert w["X"] == A[-1304:] and w["Y"] == B[:1328]
    assert w["X"] == (U.revcomp(s0[:1304]) if flags & 1 else s0[4950 - 1304:])
    assert w["Y"] == (U.revcomp(s1[3060 - 1328:]) if flags & 2 else s1[:1328])


def test_windows_clamped_to_the_unitig():
    """unitig 2 has 1,000 bases: as `from` m = P_a = 1,000 (oa + S = 1,312), as `to` n = P_b = 1,000.
    2 -> 0, + +: oa = 1000 - C_2(200) = 800, ob = C_0(800) = 792, m = 1000, n = 1304, c = 1000 - 796 = 204
    0 -> 2, + -: oa = 792, ob = 1000 - C_2(200) = 800, m = 1304, n = 1000, c = 1304 - 796 = 508
    and an ovl beyond the raw length is cut to it: 2 -> 0 with ovl 1,500: o_a = 1000, oa = 1000 - C_2(0) = 1000, o_b = 1500, ob = C_0(1500) = 1485"""
    u, cur, (s0, _, s2) = _hand()
    u["links"] = np.array([(2, 0, 800, 5, 0, 0), (0, 2, 800, 5, 2, 0), (2, 0, 1500, 6, 0, 0)], U.LINK_DT)
    w = LM.windows(u, cur, 0, 1024)
    assert (w["oa"], w["ob"], w["m"], w["n"], w["c"]) == (800, 792, 1000, 1304, 204) and w["X"] == s2 and w["Y"] == s0[:1304]
    w = LM.windows(u, cur, 1, 1024)
    assert (w["oa"], w["ob"], w["m"], w["n"], w["c"]) == (792, 800, 1304, 1000, 508) and w["X"] == s0[-1304:] and w["Y"] == U.revcomp(s2)
    w = LM.windows(u, cur, 2, 1024)
    assert (w["oa"], w["ob"], w["m"], w["n"]) == (1000, 1485, 1000, 1997) and w["c"] == 1000 - 2485 // 2


def test_twins_are_paired_in_index_order():
    L = lambda a, b, rec, f: (a, b, 800, rec, f, 0)
    links = np.array([L(0, 1, 2, 0), L(0, 2, 3, 2), L(1, 0, 2, 3), L(2, 0, 3, 2), L(3, 3, 9, 3), L(3, 3, 9, 0), L(0, 1, 4, 0), L(0, 1, 2, 0), L(1, 0, 2, 3)], U.LINK_DT)
    mate, derived = LM.pair_twins(links)
    # 0 <-> 2 (+ + / - -), 1 <-> 3 (+ - is its own shape: b + a -), the SELF pair stays unpaired, record 4 has no twin, the duplicates 7 <-> 8
    assert mate == [2, 3, 0, 1, LM.NO, LM.NO, LM.NO, 8, 7] and derived == [0, 0, 1, 1, 0, 0, 0, 0, 1]


def _mirror_case(seqs, recs, trunk=None, rounds=0):
    gm, cm, u = U.case_unitigs(seqs, recs, LC.GRAPH, LC.CLEAN)
    offs, bases = U.unitig_bases(u, seqs)
    u = dict(u, offsets=offs, bases=bases)
    cur = None
    if trunk is not None:
        cur = U.polished(u, seqs, LC.fork_table(seqs, trunk), 3)
        for _ in range(rounds):
            cur = R.realign_round(u, cur, seqs, recs, gm["contained"], cm["removed"], None)
    return u, cur


@pytest.mark.parametrize("case", ["raw", "polished", "deleted", "forged"])
def test_a_derived_twin_replays_on_its_own_windows(case):
    """the derived runs consume exactly ovl_a bases of the twin's own A^ suffix and ovl_b of its B^ prefix, every '=' column holds equal
    bases and every 'X' column different ones, and the counts are the record's"""
    kw = dict(rev="b") if case != "deleted" else dict(deleted=120)
    seqs, recs, trunk = LC.fork_case(forged=case == "forged", **kw)
    u, cur = _mirror_case(seqs, recs, trunk if case == "polished" else None)
    band0 = 256 if case == "deleted" else 512
    r = LM.align_links(u, cur, band0=band0)
    alns, ops = r["alns"], r["ops"]
    assert r["counts"]["derived"] == len(alns) // 2 and len(ops) == r["counts"]["ops"]
    seen = 0
    for k, a in enumerate(alns):
        if int(a["status"]) != LM.ALIGNED:
            assert int(a["nops"]) == 0
            continue
        w = LM.windows(u, cur, k, 4096)
        got = LM.replay(ops[int(a["op_off"]):int(a["op_off"]) + int(a["nops"])], w["X"], w["Y"], int(a["ovl_a"]), int(a["ovl_b"]))
        assert got == {f: int(a[f]) for f in ("n_eq", "n_x", "n_ins", "n_del", "score")}, k
        M = alns[int(a["mate"])]
        assert int(M["mate"]) == k and int(M["derived"]) + int(a["derived"]) == 1
        assert (int(M["ovl_a"]), int(M["ovl_b"]), int(M["n_ins"]), int(M["n_del"])) == (int(a["ovl_b"]), int(a["ovl_a"]), int(a["n_del"]), int(a["n_ins"]))
        seen += int(a["derived"])
    assert seen >= 2
    if case == "polished":
        assert cur is not None and any(int(a["n_ins"]) != int(a["n_del"]) for a in alns)     # the two sides changed length differently
    if case == "deleted":
        assert sorted(alns["band"].tolist()) == [256, 256, 512, 512] and 120 in alns["n_del"].tolist() and 120 in alns["n_ins"].tolist()
    if case == "forged":
        assert set(alns["status"].tolist()) == {LM.ALIGNED, LM.LOW_IDENTITY}


def test_the_self_case_is_never_aligned():
    seqs, recs = LC.self_case()
    u, _ = _mirror_case(seqs, recs)
    r = LM.align_links(u, None)
    st = r["alns"]["status"].tolist()
    assert st.count(LM.SELF) == 2 and r["counts"]["self"] == 2 and r["counts"]["jobs"] == 1
    for l, a in zip(u["links"], r["alns"]):
        if int(l["a"]) == int(l["b"]):
            assert int(a["status"]) == LM.SELF and int(a["mate"]) == LM.NO and int(a["band"]) == 0


# ---- the text of the L lines -----------------------------------------------------------------------------------------------------------
def _hand_gfa():
    names = ["r0", "r1", "r2"]
    u = dict(voff=np.array([0, 2, 3], np.uint64), verts=np.array([0, 3, 4], np.uint32), pos=np.array([0, 6, 0], np.uint64), nbases=np.array([6, 10, 12], np.uint32),
             len=np.array([16, 12], np.uint64), circular=np.array([0, 1], np.uint8),
             links=np.array([(0, 1, 7, 3, 0, 0), (1, 0, 7, 3, 3, 1), (0, 0, 5, 4, 1, 2), (1, 0, 9, 8, 2, 3)], U.LINK_DT))
    offs, bases = np.array([0, 16, 28], np.uint64), np.frombuffer(b"ACGTACGTACGTACGT" + b"TTTTGGGGCCCC", np.uint8)
    W = lambda op, n: n << 4 | op
    ops = np.array([W(0, 3), W(1, 1), W(0, 2), W(2, 2), W(0, 1), W(3, 1), W(0, 4),                 # link 0: 3= 1X 2= 2I 1= 1D 4=
                    W(0, 4), W(2, 1), W(0, 1), W(3, 2), W(0, 2), W(1, 1), W(0, 3)], np.uint32)     # link 1: the reversal, I and D swapped
    alns = np.zeros(4, _lib.LINK_ALN_DT)
    alns[0] = (LM.ALIGNED, 512, 7, 12, 13, 10, 1, 2, 1, 1, 0, 7, 0)
    alns[1] = (LM.ALIGNED, 512, 7, 13, 12, 10, 1, 1, 2, 0, 7, 7, 1)
    alns[2] = (LM.SELF, 0, 0, 0, 0, 0, 0, 0, 0, LM.NO, 0, 0, 0)
    alns[3] = (LM.LOW_IDENTITY, 4096, 3, 9, 9, 5, 2, 1, 1, LM.NO, 0, 0, 0)
    return names, u, offs, bases, alns, ops


def test_link_cigars_and_the_writers_lines(tmp_path):
    names, u, offs, bases, alns, ops = _hand_gfa()
    assert np.array_equal(LM.derive(ops[:7]), ops[7:])
    assert api.link_cigars(alns, ops) == [b"6M2I1M1D4M", b"4M1I1M2D6M", None, None]
    assert [LM.cigar(ops[:7]), LM.cigar(ops[7:])] == [b"6M2I1M1D4M", b"4M1I1M2D6M"]
    today = U.unitig_gfa_text(names, u, offs, bases)
    f = str(tmp_path / "u.gfa")
    api.write_unitig_gfa(f, names, u, offs, bases)
    assert open(f, "rb").read() == today                               # the default call: today's bytes
    api.write_unitig_gfa(f, names, u, offs, bases, link_alns=alns, link_ops=ops)
    got = open(f, "rb").read()
    head = today[:today.index(b"L\t")]
    want = [b"L\tutg000001l\t+\tutg000002c\t+\t6M2I1M1D4M\trc:i:3\tNM:i:4\tol:i:7\n", b"L\tutg000002c\t-\tutg000001l\t-\t4M1I1M2D6M\trc:i:3\tNM:i:4\tol:i:7\n",
            b"L\tutg000001l\t-\tutg000001l\t+\t5M\trc:i:4\n", b"L\tutg000002c\t+\tutg000001l\t-\t9M\trc:i:8\n"]
    assert got == head + b"".join(want)
    assert LM.link_lines(u, alns, ops) == want
    assert today == head + b"".join(LM.link_lines(u, np.full(4, alns[2]), ops))          # no ALIGNED link: every line is today's
    api.write_unitig_gfa(f, names, u, link_alns=alns, link_ops=ops)                       # without sequences
    assert open(f, "rb").read() == U.unitig_gfa_text(names, u)[:U.unitig_gfa_text(names, u).index(b"L\t")] + b"".join(want)
    none = dict(u, links=np.zeros(0, U.LINK_DT))
    api.write_unitig_gfa(f, names, none, offs, bases, link_alns=np.zeros(0, _lib.LINK_ALN_DT), link_ops=np.zeros(0, np.uint32))
    assert open(f, "rb").read() == U.unitig_gfa_text(names, none, offs, bases)


def test_the_dtypes_and_constants_agree():
    assert _lib.LINK_ALN_DT == LM.ALN_DT and _lib.LINK_ALN_DT.itemsize == 56
    assert (_lib.LINK_ALIGNED, _lib.LINK_EMPTY, _lib.LINK_BAND_CAPPED, _lib.LINK_LOW_IDENTITY, _lib.LINK_SELF) == (LM.ALIGNED, LM.EMPTY, LM.BAND_CAPPED, LM.LOW_IDENTITY, LM.SELF)
    assert _lib.LINK_NO_MATE == LM.NO and api.Engine.LINK_DEFAULTS == LM.DEFAULTS
