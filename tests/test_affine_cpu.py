"""CPU tests of the affine pair alignment's definition (bella_testkit/affine_mirror.py): under (1, 1, 0, 1) the
banded mirror IS the linear mirror of section 28, key for key; under four other scorings its scores equal a plain three-matrix Gotoh
written here and its runs re-score to them; hand-built pairs with their runs written out; the call-level mirror against section 28's;
the new struct and symbol against the header.  The device is held to this mirror in test_affine_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bella_amd import _lib
from bella_testkit import affine_cases as FC
from bella_testkit import affine_mirror as FM
from bella_testkit import align_cases as AC
from bella_testkit import align_mirror as AM
from bella_testkit import unitig_mirror as U
from conftest import ROOT

MODES = (AM.GLOBAL, AM.SEMIGLOBAL, AM.DOVETAIL)
NEG = -(10 ** 9)


def _pairs(count: int, top: int, seed: int):
    """seeded random and mutated pairs of 1 .. top bases"""
    rng = np.random.default_rng(seed)
    for k in range(count):
        n, m = (int(v) for v in rng.integers(1, top + 1, 2))
        Q = U.random_genome(n, 7 * seed + 3 * k)
        if k % 4 == 0:
            T = U.random_genome(m, 11 * seed + k)                      # nothing planted
        elif k % 4 == 1:
            T = AC.noisy(Q, 0.15, rng)[0]                              # a noisy copy
        elif k % 4 == 2:
            T = U.random_genome(m // 2, 13 * seed + k) + AC.noisy(Q[:max(n // 2, 1)], 0.1, rng)[0]       # a suffix of T on a prefix of Q
        else:
            T = (U.random_genome(m // 3, 17 * seed + k) + AC.noisy(Q, 0.1, rng, mix=(0.2, 0.4, 0.4))[0] + U.random_genome(m // 3, 19 * seed + k))[:top]
        yield k, Q, T


# ---- (a) the linear scoring is section 28 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_under_1_1_0_1_the_affine_mirror_is_the_linear_mirror(mode):
    """200 pairs of 1 .. 80 bases at bands of 256, 16 and 8: every key equal, ops, touch flag and the no-path dict included; a global
    pair is skipped only where the band cannot hold its start or its end"""
    seen = touched = 0
    for k, Q, T in _pairs(200, 80, 290 + mode):
        c = (len(T) - len(Q)) // 2 + (k % 5 - 2)
        for B in (256, 16, 8):
            if mode == AM.GLOBAL and not AM.feasible(mode, len(Q), len(T), c, B):
                continue
            want = AM.banded(Q, T, c, B, mode)
            got = FM.banded(Q, T, c, B, mode, (1, 1, 0, 1))
            assert got == want, (k, B, got, want)
            seen += 1
            touched += bool(want["touch"])
    assert seen >= 200 and 0 < touched < seen                          # (a band of 256 holds every pair; the narrow ones are there to touch)


# ---- (b) other scorings against a full-matrix Gotoh --------------------------------------------------------------------------------------
def gotoh(Q: bytes, T: bytes, mode: int, scoring):
    """Gotoh's three matrices over the whole rectangle, cell by cell -> (H[n], the column m of H): row 0 is one gap from (0, 0) for
    global and 0 for the other two"""
    a, b, o, e = scoring
    n, m = len(Q), len(T)
    H = [[(0 if q == 0 or mode != AM.GLOBAL else -(o + e * q)) for q in range(m + 1)]]
    E = [[NEG] * (m + 1)]
    for i in range(1, n + 1):
        h, ee, f = [NEG] * (m + 1), [NEG] * (m + 1), NEG
        for q in range(m + 1):
            ee[q] = max(H[i - 1][q] - o - e, E[i - 1][q] - e)
            f = max(h[q - 1] - o - e, f - e) if q else NEG
            d = H[i - 1][q - 1] + (a if T[q - 1] == Q[i - 1] else -b) if q else NEG
            h[q] = max(d, ee[q], f)
        H.append(h)
        E.append(ee)
    return H[n], [H[i][m] for i in range(n + 1)]


@pytest.mark.parametrize("scoring", FC.SCORINGS)
def test_the_scores_equal_a_full_matrix_gotoh_and_the_runs_rescore_to_them(scoring):
    """100 pairs of 1 .. 60 bases at a band of 256 around diagonal 0, which holds the whole rectangle: global = H[n][m]; semi-global = the
    maximum of the last row at its smallest q; dovetail = the maximum of column m at its smallest row; and in every mode the runs replay
    on the two sequences to the score, the counts and the end points"""
    for k, Q, T in _pairs(100, 60, 300 + sum(scoring)):
        for mode in MODES:
            last_row, last_col = gotoh(Q, T, mode, scoring)
            got = FM.banded(Q, T, 0, 256, mode, scoring)
            assert not got["touch"], (k, mode)
            if mode == AM.GLOBAL:
                want = (last_row[-1], len(Q), len(T))
            elif mode == AM.SEMIGLOBAL:
                want = (max(last_row), len(Q), last_row.index(max(last_row)))
            else:
                want = (max(last_col), last_col.index(max(last_col)), len(T))
            assert (got["score"], got["q_end"], got["t_end"]) == want, (k, mode)
            assert got["q_begin"] == 0 and (mode != AM.GLOBAL or got["t_begin"] == 0)
            rec = dict(q_begin=0, q_end=got["q_end"], t_begin=got["t_begin"], t_end=got["t_end"])
            back = FM.replay(AM.run_lengths(got["ops"]), Q, T, rec, scoring)
            cnt = np.bincount(np.asarray(got["ops"], np.int64), minlength=4).tolist()
            assert back == dict(n_eq=cnt[0], n_x=cnt[1], n_ins=cnt[2], n_del=cnt[3], score=got["score"]), (k, mode)


# ---- (c) hand-built pairs ------------------------------------------------------------------------------------------------------------------
def _runs(text: str):
    return [int(t[:-1]) << 4 | "=XID".index(t[-1]) for t in text.split()]


def _rl(ops):
    return np.asarray(AM.run_lengths(ops), np.int64).tolist()


@pytest.mark.parametrize("mode", MODES)
def test_a_40_base_deletion_is_one_run(mode):
    """100 bases, 40 more in the target only, 100 bases: exactly 100= 40D 100= under (1, 3, 5, 1), score 200 - 45; +1 / -1 / -1 scores
    more (160) by spreading the 40 bases over many gaps"""
    whole, cut, at = FC.one_gap(40, 100, 5)
    got = FM.banded(cut, whole, 20, 256, mode, FC.GAPPY)
    assert _rl(got["ops"]) == _runs("100= 40D 100=") and at == 100
    assert (got["score"], got["q_end"], got["t_begin"], got["t_end"], got["touch"]) == (155, 200, 0, 240, False)
    lin = FM.banded(cut, whole, 20, 256, mode, FC.LINEAR)
    assert lin["score"] == 160 and len(AM.run_lengths(lin["ops"])) > 3
    got = FM.banded(whole, cut, -20, 256, mode, FC.GAPPY)              # and the other way round: the query has them
    assert _rl(got["ops"]) == _runs("100= 40I 100=") and got["score"] == 155


@pytest.mark.parametrize("mode", MODES)
def test_the_gap_open_cost_changes_an_alignment(mode):
    c = (len(FC.OPEN_T) - len(FC.OPEN_Q)) // 2
    lin = FM.banded(FC.OPEN_Q, FC.OPEN_T, c, 256, mode, (1, 1, 0, 1))
    aff = FM.banded(FC.OPEN_Q, FC.OPEN_T, c, 256, mode, (1, 1, 6, 1))
    assert (lin["score"], _rl(lin["ops"])) == (20, _runs("12= 2D 2= 2D 10="))
    assert (aff["score"], _rl(aff["ops"])) == (10, _runs("9= 4D 3= 2X 10="))
    assert lin == AM.banded(FC.OPEN_Q, FC.OPEN_T, c, 256, mode)


def test_the_seam_cases_are_one_gap_each():
    """what test_affine_gpu.py holds the device to at every band class: the mirror returns the runs the case was built for"""
    for band0 in (256, 512, 1024, 2048):
        for length in FC.seam_lengths(band0):
            for kind in "DI":
                case, runs = FC.gap_case("global", band0, length, kind)
                bases, recs = AM.records_of(case["seqs"], case["pairs"], "global", None, case["centre"], None)
                m = FM.align(bases, recs, "global", band0, case["band_max"], scoring=FC.GAPPY)
                assert m["ops"].tolist() == runs and int(m["results"][0]["band"]) == band0, (band0, length, kind)
                assert int(m["results"][0]["score"]) == 400 - 5 - length


# ---- (d) the call-level mirror -----------------------------------------------------------------------------------------------------------
def _both(case):
    bases, recs = AM.records_of(case["seqs"], case["pairs"], case["mode"], case["rc"], case["centre"], case["overlap"])
    want = AM.align(bases, recs, case["mode"], case["band0"], case["band_max"])
    got = FM.align(bases, recs, case["mode"], case["band0"], case["band_max"], scoring=(1, 1, 0, 1))
    assert got["results"].tobytes() == want["results"].tobytes() and np.array_equal(got["ops"], want["ops"]) and got["counts"] == want["counts"]
    return got


def test_align_under_1_1_0_1_equals_section_28_on_the_edge_cases():
    E = AC.edge_cases()
    for name in sorted(E):
        _both(E[name])


@pytest.mark.parametrize("mode", AC.MODES)
def test_align_under_1_1_0_1_equals_section_28_on_mixed_lengths(mode):
    got = _both(AC.mixed_case(mode))
    assert got["counts"]["aligned"] >= 8


def test_the_budget_and_the_score_bound():
    """4 bits a cell: n * B / 2 bytes against the budget, where section 28 has n * B / 4; the score bound before any DP"""
    case, alone = FC.budget_cases("global")
    bases, recs = AM.records_of(case["seqs"], case["pairs"], "global", None, case["centre"], None)
    lin = AM.align(bases, recs, "global", 256, 4096, budget=AC.BATCH_BUDGET)["results"]
    aff = FM.align(bases, recs, "global", 256, 4096, budget=AC.BATCH_BUDGET, scoring=(1, 1, 0, 1))["results"]
    assert (aff["status"] == AM.TOO_LARGE).tolist() == [k == 5 for k in range(13)] and int(aff[5]["band"]) == 256
    for k in range(13):                                               # pairs that double to 512 need 128,000 bytes there: TOO_LARGE where section 28's 64,000 fit
        same = all(aff[k][f] == lin[k][f] for f in AM.COMPARED if f != "op_off")
        assert same or (int(aff[k]["status"]), int(aff[k]["band"]), int(lin[k]["band"])) == (AM.TOO_LARGE, 512, 512), k
    bases, recs = AM.records_of(alone["seqs"], alone["pairs"], "global", None, alone["centre"], None)
    r = FM.align(bases, recs, "global", 512, 4096, budget=AC.BATCH_BUDGET, scoring=FC.MAIN)["results"][0]
    assert (int(r["status"]), int(r["band"]), int(r["widened"])) == (AM.TOO_LARGE, 512, 0)
    recs = np.zeros(1, AM.PAIR_DT)
    recs["q_len"], recs["t_len"] = 263_200, 263_200
    r = FM.align(np.zeros(0, np.uint8), recs, scoring=(1, 255, 0, 1))["results"][0]
    assert (int(r["status"]), int(r["band"]), int(r["score"])) == (AM.TOO_LARGE, 512, 0) and 526_400 * 255 >= 1 << 27
    assert FM.too_large(1 << 26, 1 << 26, (1, 1, 0, 1)) and not FM.too_large((1 << 26) - 1, 1 << 26, (1, 1, 0, 1))
    assert FM.too_large(1 << 18, 1 << 18, (1, 3, 200, 56)) and not FM.too_large((1 << 18) - 1, 1 << 18, (1, 3, 200, 56))
    for bad in ((0, 1, 0, 1), (1, 1, 0, 0), (256, 1, 0, 1), (1, 256, 0, 1), (1, 1, 256, 1), (1, 1, 0, 256), (1, -1, 0, 1)):
        with pytest.raises(ValueError):
            FM.banded(b"A", b"A", 0, 256, AM.GLOBAL, bad)


# ---- (e) ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_the_scoring_struct_and_the_prototype_as_a_c_compiler_sees_them(tmp_path):
    cls = _lib.AlignScoring
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(bella_align_scoring));']
    for fname, _ in cls._fields_:
        src.append('printf("%s %%zu\\n", offsetof(bella_align_scoring, %s));' % (fname, fname))
    src.append('printf("abi %d\\n", BELLA_HIP_ABI_VERSION);')
    for cname in ("bella_align_params", "bella_align_pair", "bella_align_result", "bella_align_stats"):
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    protos = tmp_path / "protos.c"                                    # the prototype, as a C compiler reads it (compiled, not linked)
    protos.write_text('#include "bella_hip.h"\n'
                      'int (*run)(bella_ctx*, const uint8_t*, uint64_t, const bella_align_pair*, uint64_t, const bella_align_params*, const bella_align_scoring*,\n'
                      '           bella_align_result*, uint64_t*) = bella_hip_align_sequences_affine;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")])
    got = dict(ln.split() for ln in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 24
    assert [f for f, _ in cls._fields_] == ["struct_size", "match", "mismatch", "gap_open", "gap_extend", "reserved"]
    for fname, ftype in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset and ftype is ctypes.c_uint32, fname
    # additive: the version and the section's other structs stay what they were
    assert int(got["abi"]) == 6 and _lib.load().bella_hip_abi_version() == 6
    assert [int(got[c]) for c in ("bella_align_params", "bella_align_pair", "bella_align_result", "bella_align_stats")] == [16, 32, 64, 96]


def test_the_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bella_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(bella_hip_[A-Za-z0-9_]+)\s*\(", text))
    bound = {name: (res, args) for name, res, args in _lib.SIGNATURES}
    assert "bella_hip_align_sequences_affine" in declared and declared == set(bound)
    res, args = bound["bella_hip_align_sequences_affine"]
    assert res is ctypes.c_int and len(args) == 9 and args[6] is ctypes.POINTER(_lib.AlignScoring)
    assert hasattr(ctypes.CDLL(_lib.LIBPATH), "bella_hip_align_sequences_affine")
