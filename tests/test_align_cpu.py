"""CPU tests of the pair alignment's definition (bella_testkit/align_mirror.py): the banded mirror against a plain
full-matrix DP written here, in all three modes; its semi-global mode against realign_mirror.semiglobal_banded and its dovetail mode
against links_mirror.dovetail_banded, op for op; what the edge cases of bella_testkit/align_cases.py are built to produce; the text of
api.align_cigars; the new structs and symbols against the header.  The device is held to this mirror in test_align_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bella_amd import _lib, api
from bella_testkit import align_cases as AC
from bella_testkit import align_mirror as AM
from bella_testkit import link_cases as LC
from bella_testkit import links_mirror as LM
from bella_testkit import realign_cases as RC
from bella_testkit import realign_mirror as R
from bella_testkit import unitig_mirror as U
from conftest import ROOT


def full_matrix(Q: bytes, T: bytes, mode: int):
    """The definition without a band: every cell of the rectangle, the first of diagonal, up, left that attains the maximum, the mode's
    row 0, end and stop.  -> (score, q_end, t_begin, t_end, ops in the order of Q)"""
    n, m = len(Q), len(T)
    S = [[(-q if mode == AM.GLOBAL else 0) for q in range(m + 1)]]
    D = [[2] * (m + 1)]
    for i in range(1, n + 1):
        row, drow = [S[i - 1][0] - 1] + [0] * m, [1] + [0] * m
        for q in range(1, m + 1):
            cd, cu, cl = S[i - 1][q - 1] + (1 if T[q - 1] == Q[i - 1] else -1), S[i - 1][q] - 1, row[q - 1] - 1
            s = max(cd, cu, cl)
            row[q], drow[q] = s, (0 if s == cd else 1 if s == cu else 2)
        S.append(row)
        D.append(drow)
    if mode == AM.GLOBAL:
        i, q = n, m
    elif mode == AM.SEMIGLOBAL:
        i, q = n, S[n].index(max(S[n]))                                # the first maximum: the smallest q
    else:
        col = [S[r][m] for r in range(n + 1)]
        i, q = col.index(max(col)), m                                  # ... the smallest row
    score, q_end, t_end, ops = S[i][q], i, q, []
    while i > 0 or (mode == AM.GLOBAL and q > 0):
        d = D[i][q]
        if d == 0:
            ops.append(0 if T[q - 1] == Q[i - 1] else 1)
            i, q = i - 1, q - 1
        elif d == 1:
            ops.append(2)
            i -= 1
        else:
            ops.append(3)
            q -= 1
    return score, q_end, q, t_end, ops[::-1]


@pytest.mark.parametrize("mode", [AM.GLOBAL, AM.SEMIGLOBAL, AM.DOVETAIL])
def test_the_banded_mirror_equals_the_full_matrix(mode):
    """200 random pairs of 1 .. 80 bases at a band of 256 around diagonal 0, which holds the whole rectangle (|q - i| <= 80 < 128): score,
    end points and ops equal the plain DP's op for op, nothing touches, and the runs replay on both sequences"""
    rng = np.random.default_rng(280 + mode)
    for k in range(200):
        n, m = (int(v) for v in rng.integers(1, 81, 2))
        Q = U.random_genome(n, 10_000 + 3 * k + mode)
        if k % 4 == 0:
            T = U.random_genome(m, 20_000 + k)                         # nothing planted
        elif k % 4 == 1:
            T = AC.noisy(Q, 0.15, rng)[0]                              # a noisy copy
        elif k % 4 == 2:
            T = U.random_genome(m // 2, 30_000 + k) + AC.noisy(Q[:max(n // 2, 1)], 0.1, rng)[0]       # a suffix of T on a prefix of Q
        else:
            T = (U.random_genome(m // 3, 40_000 + k) + AC.noisy(Q, 0.1, rng)[0] + U.random_genome(m // 3, 50_000 + k))[:80]
        want = full_matrix(Q, T, mode)
        got = AM.banded(Q, T, 0, 256, mode)
        assert not got["touch"], (k, n, len(T))
        assert (got["score"], got["q_end"], got["t_begin"], got["t_end"]) == want[:4], (k, want[:4])
        assert got["q_begin"] == 0 and got["ops"] == want[4], k
        rec = dict(q_begin=0, q_end=got["q_end"], t_begin=got["t_begin"], t_end=got["t_end"])
        assert AM.replay(AM.run_lengths(got["ops"]), Q, T, rec)["score"] == got["score"]
        if mode == AM.GLOBAL:
            assert (got["q_end"], got["t_begin"], got["t_end"]) == (n, 0, len(T))
        elif mode == AM.SEMIGLOBAL:
            assert got["q_end"] == n
        else:
            assert got["t_end"] == len(T)


def test_semiglobal_mode_equals_the_realignment_mirror():
    """every read that realign_cases.line_case places on its polished unitig, as a plain pair (oriented clip, unitig, centre), at bands of
    256 and 512: the same score, end points, ops and touch flag as realign_mirror.semiglobal_banded"""
    seqs, recs = RC.line_case()
    m, c, u = U.case_unitigs(seqs, recs, RC.GRAPH, {})
    p = U.polished(u, seqs, RC.line_table(seqs), 3)
    pl, _ = R.place(u, p, [len(s) for s in seqs], recs, m["contained"], c["removed"], None, 256, 2048)
    offs = p["offsets"].astype(np.int64)
    cb = bytes(p["bases"].tobytes() if hasattr(p["bases"], "tobytes") else p["bases"])
    seen = touched = 0
    for r in np.flatnonzero(pl["status"] == R.VOTED).tolist():
        k = int(pl[r]["unitig"])
        read = U.revcomp(seqs[r]) if int(pl[r]["orient"]) else seqs[r]
        utg = cb[int(offs[k]):int(offs[k + 1])]
        centre = int(pl[r]["s"]) + ((int(pl[r]["e"]) - int(pl[r]["s"])) - len(read)) // 2
        for B in (256, 512):
            want = R.semiglobal_banded(read, utg, centre, B)
            got = AM.banded(read, utg, centre, B, AM.SEMIGLOBAL)
            assert got["touch"] == want["touch"] and got["ops"] == want["ops"], (r, B)
            if want["ops"] is not None:
                assert (got["score"], got["t_begin"], got["t_end"], got["q_end"]) == (want["score"], want["q_begin"], want["q_end"], len(read)), (r, B)
            seen += 1
            touched += bool(want["touch"])
    assert seen >= 20 and 0 < touched < seen


@pytest.mark.parametrize("kw", [dict(rev="b"), dict(deleted=120), dict(forged=True, rev="b")])
def test_dovetail_mode_equals_the_link_mirror(kw):
    """the windows of link_cases.fork_case's links as plain pairs (rows Y, columns X, centre), at bands of 256 and 512: the same score,
    end row, start column, ops and touch flag as links_mirror.dovetail_banded"""
    seqs, recs, _ = LC.fork_case(**kw)
    _, _, u = U.case_unitigs(seqs, recs, LC.GRAPH, LC.CLEAN)
    offs, bases = U.unitig_bases(u, seqs)
    u = dict(u, offsets=offs, bases=bases)
    assert len(u["links"]) >= 4
    for k in range(len(u["links"])):
        w = LM.windows(u, None, k, 4096)
        for B in (256, 512):
            want = LM.dovetail_banded(w["X"], w["Y"], w["c"], B)
            got = AM.banded(w["Y"], w["X"], w["c"], B, AM.DOVETAIL)
            assert got["touch"] == want["touch"] and got["ops"] == want["ops"], (k, B)
            if want["ops"] is not None:
                assert (got["score"], got["q_end"], got["t_begin"], got["t_end"]) == (want["score"], want["i_end"], want["q_begin"], w["m"]), (k, B)


def _mirror(case, **kw):
    bases, recs = AM.records_of(case["seqs"], case["pairs"], case["mode"], case["rc"], case["centre"], case["overlap"])
    return AM.align(bases, recs, case["mode"], case["band0"], case["band_max"], **kw)


def test_the_edge_cases_produce_what_they_were_built_for():
    E = AC.edge_cases()
    one = lambda name: (_mirror(E[name])["results"][0], _mirror(E[name])["counts"])
    r, cnt = one("global_start_outside_the_first_band")
    assert (int(r["status"]), int(r["band"]), int(r["widened"]), cnt["repeated"], cnt["dp_cells"]) == (AM.ALIGNED, 512, 1, 0, 500 * 512)
    assert (int(r["n_del"]), int(r["n_eq"]), int(r["score"])) == (300, 500, 200)
    r, cnt = one("global_capped_before_any_dp")
    assert (int(r["status"]), int(r["band"]), int(r["widened"]), cnt["dp_cells"], int(r["score"]), int(r["nops"])) == (AM.BAND_CAPPED, 512, 1, 0, 0, 0)
    for mode in ("global", "semiglobal"):
        r, cnt = one("block_120_doubles_the_band_" + mode)
        assert (int(r["status"]), int(r["band"]), int(r["widened"]), cnt["repeated"], int(r["n_ins"])) == (AM.ALIGNED, 512, 1, 1, 120), mode
        r, cnt = one("block_248_is_capped_at_512_" + mode)
        assert (int(r["status"]), int(r["band"]), int(r["n_eq"])) == (AM.BAND_CAPPED, 512, 0), mode
    r, _ = one("dovetail_best_cell_in_row_0")
    assert (int(r["status"]), int(r["nops"]), int(r["score"]), int(r["q_end"]), int(r["t_begin"]), int(r["t_end"])) == (AM.ALIGNED, 0, 0, 0, 300, 300)
    r, _ = one("one_base_match_global")
    assert (int(r["score"]), int(r["n_eq"]), int(r["nops"])) == (1, 1, 1)
    r, _ = one("one_base_mismatch_global")
    assert (int(r["score"]), int(r["n_x"])) == (-1, 1)
    r, _ = one("one_against_600_global")                               # centre 299: the start fits from a band of 1,024 on
    assert (int(r["status"]), int(r["band"]), int(r["widened"]), int(r["n_del"])) == (AM.ALIGNED, 1024, 2, 599)
    r, _ = one("identical_global")
    assert (int(r["score"]), int(r["nops"])) == (500, 1)
    r, _ = one("nothing_in_common_global")
    assert int(r["score"]) == -300
    for mode in AC.MODES:
        r, _ = one("centre_off_by_100_" + mode)
        assert int(r["status"]) == AM.ALIGNED and int(r["n_eq"]) > 100, mode
    # a pair that is too large for the budget, and one that is too large whatever the budget
    c = AC.batch_case("global")
    res = _mirror(c, budget=AC.BATCH_BUDGET)["results"]
    assert (res["status"] == AM.TOO_LARGE).tolist() == [k == 5 for k in range(13)] and int(res[5]["band"]) == 256
    recs = np.zeros(1, AM.PAIR_DT)
    recs["q_len"], recs["t_len"] = 1 << 26, 1 << 26
    r = AM.align(np.zeros(0, np.uint8), recs)["results"][0]
    assert (int(r["status"]), int(r["band"])) == (AM.TOO_LARGE, 512)


def test_records_of_supplies_the_wrappers_defaults():
    _, recs = AM.records_of([b"A" * 10, b"C" * 25, b"G" * 7], [(0, 1), (1, 2), (2, 1)], "global")
    assert recs["centre"].tolist() == [7, -9, 9] and recs["q_off"].tolist() == [0, 10, 35] and recs["t_len"].tolist() == [25, 7, 25]
    _, recs = AM.records_of([b"A" * 10, b"C" * 25], [(0, 1)], "dovetail", rc=True, overlap=6)
    assert recs["centre"].tolist() == [19] and recs["flags"].tolist() == [AM.PAIR_RC]
    assert AM.default_centre(10, 3) == -4                              # floor, not truncation


def test_align_cigars():
    res = np.zeros(3, _lib.ALIGN_RES_DT)
    ops = np.array([5 << 4 | 0, 1 << 4 | 1, 2 << 4 | 0, 3 << 4 | 2, 4 << 4 | 0, 7 << 4 | 3], np.uint32)
    res["status"] = [_lib.ALIGN_ALIGNED, _lib.ALIGN_BAND_CAPPED, _lib.ALIGN_ALIGNED]
    res["op_off"], res["nops"] = [0, 0, 6], [6, 0, 0]
    assert api.align_cigars(res, ops) == [b"5=1X2=3I4=7D", None, b""]
    assert api.align_cigars(res, ops, eqx=False) == [b"8M3I4M7D", None, b""]


def test_align_structs_equal_the_header_as_a_c_compiler_sees_them(tmp_path):
    structs = {"bella_align_params": _lib.AlignParams, "bella_align_pair": _lib.AlignPair, "bella_align_result": _lib.AlignResult, "bella_align_stats": _lib.AlignStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            src.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    src.append('printf("abi version %d\\n", BELLA_HIP_ABI_VERSION);')
    src.append('printf("mode values %d\\n", BELLA_ALIGN_GLOBAL + 10 * BELLA_ALIGN_SEMIGLOBAL + 100 * BELLA_ALIGN_DOVETAIL);')
    src.append('printf("status values %d\\n", BELLA_ALIGN_STATUS_ALIGNED + 10 * BELLA_ALIGN_STATUS_BAND_CAPPED + 100 * BELLA_ALIGN_STATUS_TOO_LARGE);')
    src.append('printf("band values %d\\n", BELLA_ALIGN_DEFAULT_BAND + BELLA_ALIGN_DEFAULT_BAND_MAX + BELLA_ALIGN_MAX_BAND + (int)BELLA_ALIGN_PAIR_RC);')
    for cname in ("bella_link_params", "bella_link_aln", "bella_link_stats", "bella_trace"):
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    protos = tmp_path / "protos.c"                                    # the prototypes, as a C compiler reads them (compiled, not linked)
    protos.write_text('#include "bella_hip.h"\n'
                      'int (*run)(bella_ctx*, const uint8_t*, uint64_t, const bella_align_pair*, uint64_t, const bella_align_params*, bella_align_result*, uint64_t*) = bella_hip_align_sequences;\n'
                      'int (*ops)(bella_ctx*, uint32_t*, uint64_t) = bella_hip_get_align_ops;\n'
                      'int (*st)(bella_ctx*, void*, uint64_t) = bella_hip_get_align_stats;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert [ctypes.sizeof(c) for c in structs.values()] == [16, 32, 64, 96]
    for dt, cls in ((_lib.ALIGN_PAIR_DT, _lib.AlignPair), (_lib.ALIGN_RES_DT, _lib.AlignResult)):
        assert dt.itemsize == ctypes.sizeof(cls) and all(dt.fields[f][1] == getattr(cls, f).offset for f, _ in cls._fields_)
    assert _lib.ALIGN_PAIR_DT == AM.PAIR_DT and _lib.ALIGN_RES_DT == AM.RES_DT
    assert got[("mode", "values")] == 210 and got[("status", "values")] == 210 and got[("band", "values")] == 512 + 4096 + 16384 + 1
    assert (_lib.ALIGN_GLOBAL, _lib.ALIGN_SEMIGLOBAL, _lib.ALIGN_DOVETAIL) == (AM.GLOBAL, AM.SEMIGLOBAL, AM.DOVETAIL) == (0, 1, 2)
    assert (_lib.ALIGN_ALIGNED, _lib.ALIGN_BAND_CAPPED, _lib.ALIGN_TOO_LARGE) == (AM.ALIGNED, AM.BAND_CAPPED, AM.TOO_LARGE) == (0, 1, 2)
    assert _lib.ALIGN_MODES == AM.MODES and _lib.ALIGN_PAIR_RC == AM.PAIR_RC == 1
    # additive: the version and the neighbouring structs stay what they were
    assert got[("abi", "version")] == 6 and _lib.load().bella_hip_abi_version() == 6
    assert got[("bella_link_params", "size")] == ctypes.sizeof(_lib.LinkParams) == 16 and got[("bella_link_stats", "size")] == ctypes.sizeof(_lib.LinkStats)
    assert got[("bella_link_aln", "size")] == _lib.LINK_ALN_DT.itemsize == 56 and got[("bella_trace", "size")] == _lib.TRACE_DT.itemsize == 56


def test_every_declared_symbol_is_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bella_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bella_hip_[A-Za-z0-9_]+)\s*\(", text))
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert {"bella_hip_align_sequences", "bella_hip_get_align_ops", "bella_hip_get_align_stats"} <= declared
    assert declared == bound, declared ^ bound
    lib = ctypes.CDLL(_lib.LIBPATH)
    for name in sorted(declared):
        assert hasattr(lib, name), name
