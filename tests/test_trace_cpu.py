"""CPU tests of the traced alignments: the numpy mirrors (full rectangle and banded) against scalar DPs, the
replay checker, the hand-made case list of the banded GPU tests, the true-PAF writer (plain host code), the command line's --cigar
rules and the ABI additions.  No device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bella_amd import _lib, api
from bella_testkit import trace_cases as T
from bella_testkit import trace_mirror as M
from conftest import ROOT


def _brute(h, v):
    """the definition, cell by cell: (score, i, j) of the best cell, ties to the smallest i + j, then the smallest i"""
    n, m = len(v), len(h)
    S = [[0] * (m + 1) for _ in range(n + 1)]
    best = (0, 0, 0)
    cells = []
    for i in range(n + 1):
        for j in range(m + 1):
            if i or j:
                c = []
                if i and j:
                    c.append(S[i - 1][j - 1] + (1 if v[i - 1] == h[j - 1] else -1))
                if i:
                    c.append(S[i - 1][j] - 1)
                if j:
                    c.append(S[i][j - 1] - 1)
                S[i][j] = max(c)
            cells.append((-S[i][j], i + j, i, j))
    s, _, i, j = min(cells)
    return -s, i, j


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n).tolist())


def test_mirror_equals_the_scalar_dp():
    """a few hundred random short extensions: related sequences, unrelated ones, empty sides, one-sided rectangles, all-mismatch"""
    rng = np.random.default_rng(3)
    cases = [(b"", b""), (b"ACGT", b""), (b"", b"ACGT"), (b"AAAA", b"CCCC"), (b"A", b"A"), (b"ACGTACGT", b"ACGTACGT"), (b"AAAAAAAA", b"A")]
    for t in range(400):
        n, m = int(rng.integers(0, 30)), int(rng.integers(0, 30))
        v = _rand(rng, n)
        if t % 3 == 0:
            h = _rand(rng, m)
        elif t % 3 == 1:                        # v with errors: substitutions, insertions, deletions
            out = []
            for c in v:
                u = rng.random()
                if u < 0.1:
                    continue
                out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))) if u < 0.2 else c)
                if u > 0.9:
                    out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
            h = bytes(out)
        else:
            h = _rand(rng, m, b"AC")
        cases.append((h, v))
    for h, v in cases:
        assert M.extension_optimum(h, v) == _brute(h, v), (h, v)


def test_trace_expect_on_both_strands():
    """the pair-level mirror: seed placement on the reverse-complemented H, rectangles clamped to the reads, left part reversed"""
    rng = np.random.default_rng(4)
    k = 5
    for t in range(60):
        core = _rand(rng, 60)
        V = _rand(rng, int(rng.integers(0, 8))) + core + _rand(rng, int(rng.integers(0, 8)))
        Hf = _rand(rng, int(rng.integers(0, 8))) + core + _rand(rng, int(rng.integers(0, 8)))
        strand = t & 1
        H = M.revcomp(Hf) if strand else Hf
        sVcore = int(rng.integers(0, 60 - k + 1))
        sV = V.index(core) + sVcore
        sHo = Hf.index(core) + sVcore                      # on the oriented H
        seedH = len(H) - sHo - k if strand else sHo
        aln = dict(begH=int(rng.integers(0, sHo + 1)), endH=int(rng.integers(sHo + k, len(H) + 1)), begV=int(rng.integers(0, sV + 1)),
                   endV=int(rng.integers(sV + k, len(V) + 1)), strand=strand)
        e = M.trace_expect(H, V, seedH, sV, k, aln)
        Hp = M.oriented(H, strand)
        sl, il, jl = _brute(Hp[aln["begH"]:sHo][::-1], V[aln["begV"]:sV][::-1])
        sr, ir, jr = _brute(Hp[sHo + k:aln["endH"]], V[sV + k:aln["endV"]])
        assert e == dict(score=sl + k + sr, tbegH=sHo - jl, tbegV=sV - il, tendH=sHo + k + jr, tendV=sV + k + ir)
        assert aln["begH"] <= e["tbegH"] and e["tendH"] <= aln["endH"] and aln["begV"] <= e["tbegV"] and e["tendV"] <= aln["endV"]


def test_replay_checker_rejects_wrong_op_lists():
    H, V = b"ACGTACGTAC", b"ACGTTCGAC"
    good = M.parse_cigar("4=1X2=1D2=")
    assert M.replay(good, H, V, 0, 10, 0, 9) == dict(n_eq=8, n_x=1, n_ins=0, n_del=1, score=6)
    assert M.cigar(good) == "4=1X2=1D2=" and M.cigar(good, reverse=True) == "2=1D2=1X4="
    for bad, why in (("4=1X2=1D1=1=", "merged"), ("5=2=1D2=", "merged"), ("4=1X2=1D3=", "leave"), ("4=1X2=1I2=", "leave"), ("4=1X2=1D1=", "end at"),
                     ("5=1X1=1D2=", "'=' over a mismatch"), ("4=2X1=1D2=", "'X' over a match"), ("4=1X2=2=", "merged"), ("4=1X2=1D", "end at")):
        with pytest.raises(ValueError, match=why):
            M.replay(M.parse_cigar(bad), H, V, 0, 10, 0, 9)
    with pytest.raises(ValueError, match="empty"):
        M.replay(np.array([4 << 4, 0 << 4 | 1, 5 << 4], np.uint32), H, V, 0, 9, 0, 9)
    with pytest.raises(ValueError, match="unknown op"):
        M.replay(np.array([4 << 4 | 7], np.uint32), H, V, 0, 4, 0, 4)
    with pytest.raises(ValueError, match="n_x"):            # counters of a record that disagree with its ops
        rec = np.zeros(1, _lib.TRACE_DT)[0]
        rec["nops"], rec["tendH"], rec["tendV"], rec["n_eq"], rec["n_x"], rec["n_del"], rec["score"] = 5, 10, 9, 8, 2, 1, 6
        M.check_trace(rec, good, H, V, 0)


def _records():
    names = ["readA", "readB", "readC"]
    seqs = [b"ACGTACGTACGTAAAC", b"ACGTACGTTCGTAAAC", M.revcomp(b"GGACGTACGTACGTAAAC")]
    lens = [len(s) for s in seqs]
    pairs = np.zeros(3, _lib.PAIR_DT)
    alns = np.zeros(3, _lib.ALN_DT)
    tr = np.zeros(3, _lib.TRACE_DT)
    # pair 0: H = readB (rid 1), V = readA (cid 0), strand n: 8= 1X 7=
    pairs[0] = (1, 0, 3, 4, 4, 1)
    alns[0] = (10, 0, 16, 0, 16, 16, 0, 1, 0, 0)
    # pair 1: H = readC (rid 2), V = readA (cid 0), strand c: a hand-made trace from H' 2 to 18 with one I and one D (3=1I2=1D10=)
    pairs[1] = (2, 0, 3, 4, 4, 2)
    alns[1] = (12, 1, 18, 0, 16, 17, 1, 1, 0, 0)
    # pair 2: failed alignment: no line
    pairs[2] = (2, 1, 1, 2, 2, 1)
    alns[2] = (1, 0, 5, 0, 5, 9, 0, 0, 0, 0)
    ops = np.concatenate([M.parse_cigar("8=1X7="), M.parse_cigar("3=1I2=1D10=")])
    tr[0] = (0, 3, 256, 14, 0, 16, 0, 16, 15, 1, 0, 0, 0)
    tr[1] = (3, 5, 256, 13, 2, 18, 0, 16, 15, 0, 1, 1, 0)
    return names, lens, pairs, alns, tr, ops


def test_traced_writer_lines_both_strands(tmp_path):
    """bella_hip_write_output_traced on hand-made records: the expected lines on both strands ('-': H coordinates on the original
    strand, runs reversed), failed and untraced pairs give no line, the file is appended to, measured bytes = written bytes"""
    names, lens, pairs, alns, tr, ops = _records()
    want = (b"readA\t16\t0\t16\t+\treadB\t16\t0\t16\t15\t16\t255\tAS:i:10\tov:i:16\tNM:i:1\tcg:Z:8=1X7=\n"
            b"readA\t16\t0\t16\t-\treadC\t18\t0\t16\t15\t17\t255\tAS:i:12\tov:i:17\tNM:i:2\tcg:Z:10=1D2=1I3=\n")
    f = str(tmp_path / "t.paf")
    for nt in (1, 3, 0):
        open(f, "wb").write(b"head\n")
        st = api.write_output_traced(f, api.BellaPars(kmerSize=4, outputPaf=True), names, lens, pairs, alns, tr, ops, nthreads=nt)
        data = open(f, "rb").read()
        assert data == b"head\n" + want
        assert st.lines == 2 and st.bytes == len(want) and st.aligned_pairs == 3
    assert api.cigar_strings(tr, ops, reverse=alns["strand"] == 1) == ["8=1X7=", "10=1D2=1I3=", ""]
    tr[0]["nops"] = 0                                     # untraced: no line
    open(f, "wb").close()
    st = api.write_output_traced(f, api.BellaPars(kmerSize=4, outputPaf=True), names, lens, pairs, alns, tr, ops)
    assert open(f, "rb").read() == want.split(b"\n", 1)[1] and st.lines == 1
    # many records over several threads: every share's measured size is its written size (the writer reports a mismatch as an error)
    big = 70000
    P, A, T = np.repeat(pairs[:2], big // 2), np.repeat(alns[:2], big // 2), np.repeat(tr[:2], big // 2)
    open(f, "wb").close()
    st = api.write_output_traced(f, api.BellaPars(kmerSize=4, outputPaf=True), names, lens, P, A, T, ops, nthreads=4)
    assert st.lines == big // 2 and os.path.getsize(f) == st.bytes == (big // 2) * len(want.split(b"\n", 1)[1]) and st.threads > 1
    with pytest.raises(api.BellaHipError):
        api.write_output_traced(f, api.BellaPars(kmerSize=4, skipAlignment=True), names, lens, pairs, alns, tr, ops)


def test_traced_writer_with_no_pairs_and_with_a_bad_record(tmp_path):
    """a stage without pairs appends nothing and succeeds, with or without arrays (as bella_hip_write_output does); a record whose
    runs lie outside the ops array is refused before the file is touched"""
    names, lens, pairs, alns, tr, ops = _records()
    f = str(tmp_path / "e.paf")
    open(f, "wb").write(b"head\n")
    pars = api.BellaPars(kmerSize=4, outputPaf=True)
    st = api.write_output_traced(f, pars, names, lens, pairs[:0], alns[:0], tr[:0], ops[:0])
    assert st.lines == 0 and st.bytes == 0 and open(f, "rb").read() == b"head\n"
    st = api.write_output(f, pars, names, lens, pairs[:0], alns[:0])
    assert st.lines == 0 and open(f, "rb").read() == b"head\n"
    lib = _lib.load()
    cp = pars.c()
    assert lib.bella_hip_write_output_traced(f.encode(), ctypes.byref(cp), 0, None, None, None, None, None, None, 0, 0, 1, None) == 0
    assert open(f, "rb").read() == b"head\n"
    bad = tr.copy()
    bad[1]["op_off"] = len(ops) - 2                         # 5 runs from there: past the end
    with pytest.raises(api.BellaHipError):
        api.write_output_traced(f, pars, names, lens, pairs, alns, bad, ops)
    assert open(f, "rb").read() == b"head\n"


def test_cli_cigar_rules_without_a_device(tmp_path):
    from bella_amd import build as b
    exe = b.build_cli()
    run = lambda args: subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    p = run(["--help"])
    assert p.returncode == 0 and b"--cigar" in p.stdout and b"--trace-band" in p.stdout
    for bad in (["--cigar"], ["--cigar", "--paf", "--skip-alignment"], ["--cigar", "--skip-alignment"], ["--paf", "--trace-band", "512"],
                ["--paf", "--cigar", "--trace-band", "-4"]):
        p = run(["-f", "in.txt", "-o", "x"] + bad)
        assert p.returncode == 1 and b"bella-hip:" in p.stderr and (b"--cigar" in p.stderr or b"--trace-band" in p.stderr), (bad, p.stderr)
    for bad in (["--cigar"], ["--cigar", "--paf", "--skip-alignment"]):
        assert b"--cigar" in run(["-f", "in.txt", "-o", "x"] + bad).stderr


def test_trace_structs_as_a_c_compiler_sees_them(tmp_path):
    """sizeof / offsetof of bella_trace and bella_trace_stats from gcc against the numpy / ctypes mirrors; the ABI version stays 6 and
    the library exports the new entry points"""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {',
           'printf("bella_trace size %zu\\n", sizeof(bella_trace));', 'printf("bella_trace_stats size %zu\\n", sizeof(bella_trace_stats));',
           'printf("default band %d\\n", BELLA_TRACE_DEFAULT_BAND);']
    for f in _lib.TRACE_DT.names:
        src.append('printf("bella_trace %s %%zu\\n", offsetof(bella_trace, %s));' % (f, f))
    for f, _ in _lib.TraceStats._fields_:
        src.append('printf("bella_trace_stats %s %%zu\\n", offsetof(bella_trace_stats, %s));' % (f, f))
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    assert got[("bella_trace", "size")] == _lib.TRACE_DT.itemsize == 56
    assert got[("bella_trace_stats", "size")] == ctypes.sizeof(_lib.TraceStats)
    for f in _lib.TRACE_DT.names:
        assert got[("bella_trace", f)] == _lib.TRACE_DT.fields[f][1], f
    for f, _ in _lib.TraceStats._fields_:
        assert got[("bella_trace_stats", f)] == getattr(_lib.TraceStats, f).offset, f
    assert got[("default", "band")] in (256, 512, 1024)
    lib = _lib.load()
    assert lib.bella_hip_abi_version() == 6
    for name in ("bella_hip_trace_pairs", "bella_hip_get_traces", "bella_hip_trace_batch", "bella_hip_get_batch_ops", "bella_hip_get_trace_stats", "bella_hip_write_output_traced"):
        assert hasattr(lib, name), name


# ---- the banded mirror -----------------------------------------------------------------------------------------------------------
def _brute_banded(h, v, B):
    """the banded definition, cell by cell: (score, (i, j), ops far end first, touch, the cells that hold the best score)"""
    n, m, half = len(v), len(h), B // 2
    rows = min(n, m + half)
    S, D = {(0, 0): 0}, {}
    for i in range(rows + 1):
        for j in range(m + 1):
            if not 0 <= j - i + half < B or (i == 0 and j == 0):
                continue
            c = []                                           # in the order of preference: diagonal, up, left
            if (i - 1, j - 1) in S:
                c.append((S[i - 1, j - 1] + (1 if v[i - 1] == h[j - 1] else -1), 0))
            if (i - 1, j) in S:
                c.append((S[i - 1, j] - 1, 1))
            if (i, j - 1) in S:
                c.append((S[i, j - 1] - 1, 2))
            S[i, j] = max(x for x, _ in c)
            D[i, j] = next(d for x, d in c if x == S[i, j])
    _, _, bi, bj = min((-s, i + j, i, j) for (i, j), s in S.items())
    ops, touch = [], 0
    i, j = bi, bj
    while i or j:
        p = j - i + half
        touch |= (M.TOUCH_LOW if p <= 0 else 0) | (M.TOUCH_HIGH if p >= B - 1 else 0)
        d = 2 if i == 0 else 1 if j == 0 else D[i, j]
        if d == 0:
            ops.append(0 if h[j - 1] == v[i - 1] else 1)
        else:
            ops.append(d + 1)
        i, j = i - (d != 2), j - (d != 1)
    return S[bi, bj], (bi, bj), ops, touch, sorted(c for c, s in S.items() if s == S[bi, bj])


def _mutated(rng, v, rate):
    out = []
    for c in v:
        u = rng.random()
        if u < rate:
            continue
        out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))) if u < 2 * rate else c)
        if u > 1 - rate:
            out.append(int(rng.choice(np.frombuffer(b"ACGT", np.uint8))))
    return bytes(out)


def test_banded_mirror_equals_the_scalar_banded_dp():
    """score, best cell, every op of the walk and the touched edges, on bands of 2 .. 32 diagonals: random, related, empty sides,
    n >> m, m >> n, homopolymers, dinucleotide repeats.  Small bands put most paths on an edge and most cells into a tie."""
    rng = np.random.default_rng(31)
    cases = [(b"", b""), (b"ACGT", b""), (b"", b"ACGT"), (b"AAAA", b"CCCC"), (b"A", b"A"), (b"ACGTACGT", b"ACGTACGT"), (b"A" * 40, b"A"), (b"A", b"A" * 40),
             (b"A" * 30, b"A" * 22), (b"A" * 19, b"A" * 33), (b"AC" * 15, b"AC" * 11), (b"AC" * 9 + b"A", b"CA" * 14), (b"ACG" * 8, b"ACG" * 12 + b"T"),
             (b"A" * 10 + b"C" + b"A" * 12, b"A" * 14 + b"C" + b"A" * 9)]
    for t in range(360):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        kind = t % 6
        if kind == 0:
            h, v = _rand(rng, m), _rand(rng, n)
        elif kind == 1:
            v = _rand(rng, n)
            h = _mutated(rng, v, 0.1)
        elif kind == 2:
            h, v = _rand(rng, m, b"AC"), _rand(rng, n, b"AC")
        elif kind == 3:                          # n >> m
            v = _rand(rng, 40 + n)
            h = _mutated(rng, v[:int(rng.integers(0, 6))], 0.1)
        elif kind == 4:                          # m >> n
            h = _rand(rng, 40 + m)
            v = _mutated(rng, h[:int(rng.integers(0, 6))], 0.1)
        else:                                    # one gap of a few bases inside a repeat
            u = [b"A", b"AC", b"GAT"][t % 3]
            v = u * (n // len(u)) + b"T" + u * (m // len(u))
            h = u * (m // len(u)) + b"T" + u * (n // len(u))
        cases.append((h, v))
    bands, touched, tied = set(), 0, 0
    for q, (h, v) in enumerate(cases):
        for B in {2, 32, 2 * int(rng.integers(1, 17)), 2 * int(rng.integers(1, 17))}:
            want = _brute_banded(h, v, B)
            assert M.banded_extension(h, v, B) == want[:4], (h, v, B)
            bands.add(B)
            touched += bool(want[3])
            tied += len(want[4]) > 1
    assert bands == set(range(2, 33, 2)) and touched > 200 and tied > 200
    with pytest.raises(ValueError):
        M.banded_extension(b"A", b"A", 3)


def test_banded_mirror_on_the_covering_band_is_the_full_rectangle():
    """B = the covering band: score and best cell are extension_optimum's, and nothing touches unless the path runs along an axis"""
    rng = np.random.default_rng(32)
    for t in range(40):
        v = _rand(rng, int(rng.integers(0, 200)))
        h = _mutated(rng, v, 0.08) if t % 2 else _rand(rng, int(rng.integers(0, 200)))
        B = M.trace_cover_band(len(v), len(h))
        assert B >= 2 * max(len(v), len(h) + 1) and (B == 256 or B // 2 < 2 * max(len(v), len(h) + 1))
        s, cell, ops, touch = M.banded_extension(h, v, B)
        assert (s, *cell) == M.extension_optimum(h, v), (h, v)
        assert not touch
    assert [M.first_band(b) for b in (0, 1, 256, 257, 300, 512, 1024, 2048, 1 << 18, 1 << 20)] == [256, 256, 256, 512, 512, 512, 1024, 2048, 1 << 18, 1 << 18]


@pytest.fixture(scope="module")
def listed():
    cases = T.build_cases()
    return cases, T.expectations(cases)


def test_case_list_is_deterministic_and_its_reads_hit_every_packed_offset():
    a, b = T.build_cases(), T.build_cases()
    assert [(c.name, c.H, c.V, c.seedH, c.seedV, c.strand, c.aln) for c in a] == [(c.name, c.H, c.V, c.seedH, c.seedV, c.strand, c.aln) for c in b]
    assert len({c.name for c in a}) == len(a)
    rs = T.read_set(a)
    assert rs.nreads == 2 * len(a) and not (rs.lengths % 16 == 0).any() and int(rs.lengths.max()) <= 4500
    assert set((rs.offsets[:-1] % 16).tolist()) == set(range(16))
    assert {c.strand for c in a} == {0, 1}
    for c in a:                                              # the seed lies in both reads, the rectangle in the reads
        sH, (ml, nl), (mr, nr) = M.rectangles(len(c.H), len(c.V), c.seedH, c.seedV, T.K, c.aln)
        assert 0 <= c.seedH <= len(c.H) - T.K and 0 <= c.seedV <= len(c.V) - T.K
        assert (ml, nl, mr, nr) == (sH - c.aln["begH"], c.seedV - c.aln["begV"], c.aln["endH"] - sH - T.K, c.aln["endV"] - c.seedV - T.K)
    by = {c.name: c for c in a}
    assert by["tall0_right0"].seedV == 0 and by["tall1_left0"].seedV == len(by["tall1_left0"].V) - T.K      # a seed at position 0 and at len - k


def test_case_list_meets_its_coverage_conditions(listed):
    """on the mirror alone: what the GPU test of the list relies on to reach every kernel below its cover, both edges, every widening"""
    cases, expect = listed
    cov = T.coverage(cases, expect)
    print("TRACE case list: %d cases; side DPs taller than their band %s; touches (low, high) %s; short without widening %d; bookkeeping %s"
          % (len(cases), cov["tall"], cov["touches"], cov["short"], {b0: T.bookkeeping(expect[b0]) for b0 in T.BAND0S}))
    T.check_coverage(cov)
    e0 = {c.name: expect[0][q] for q, c in enumerate(cases)}
    ec = {c.name: expect[T.BAND0S[-1]][q] for q, c in enumerate(cases)}
    for total, last in ((130, 512), (260, 1024), (520, 2048)):           # the drift families widen step by step, on either edge, up to the optimum
        for on, edge in (("V", M.TOUCH_LOW), ("H", M.TOUCH_HIGH)):
            for name, sd in (("drift%d%s_right0" % (total, on), 1), ("drift%d%s_left1" % (total, on), 0)):
                rec, _, steps = e0[name]
                assert [b for b, _ in steps[sd]] == [256 << s for s in range(rec["widened"] + 1)] and steps[sd][-1] == (last, 0), (name, steps)
                assert all(t == edge for _, t in steps[sd][:-1]) and all(s == (256, 0) for s in steps[1 - sd]) and len(steps[0]) == len(steps[1])
                assert rec["score"] == ec[name][0]["score"] and rec["band"] == last
    assert e0["drift_both130_0"][2] == ([(256, M.TOUCH_LOW), (512, 0)], [(256, M.TOUCH_HIGH), (512, 0)])          # two doublings, one repeat
    assert e0["drift_130H_260V_1"][2] == ([(256, M.TOUCH_HIGH), (512, 0), (512, 0)], [(256, M.TOUCH_LOW), (512, M.TOUCH_LOW), (1024, 0)])
    assert T.bookkeeping(expect[0])["widened_extensions"] > T.bookkeeping(expect[0])["repeated_pairs"]
    rec, _, steps = e0["block128V_right0"]                               # 128 reaches p = 0 and widens; 140 stays inside, short of the optimum
    assert steps[1] == [(256, M.TOUCH_LOW), (512, 0)] and rec["score"] == ec["block128V_right0"][0]["score"]
    rec, _, steps = e0["block140V_right1"]
    assert steps == ([(256, 0)], [(256, 0)]) and rec["widened"] == 0 and rec["score"] < ec["block140V_right1"][0]["score"] - 300
    # the two co-optimal cells of tie_shift lie on one anti-diagonal: the smaller i wins
    c = next(c for c in cases if c.name == "tie_shift_right0")
    sH, _, (mr, nr) = M.rectangles(len(c.H), len(c.V), c.seedH, c.seedV, T.K, c.aln)
    s, cell, _, _, cells = _brute_banded(c.H[sH + T.K:sH + T.K + mr], c.V[c.seedV + T.K:c.seedV + T.K + nr], 256)
    assert len(cells) == 2 and sum(cells[0]) == sum(cells[1]) and cell == cells[0] and M.banded_extension(c.H[sH + T.K:sH + T.K + mr], c.V[c.seedV + T.K:c.seedV + T.K + nr], 256)[1] == cell


def test_pair_level_ops_replay_with_the_records_counters(listed):
    """every case at every first band: the op words replay on the reads between the record's end points, and counters and score
    are the ops' own; the seams are merged (replay refuses two adjacent runs with one op)"""
    cases, expect = listed
    merged = 0
    for b0 in T.BAND0S:
        for c, (rec, ops, steps) in zip(cases, expect[b0]):
            got = M.replay(ops, M.oriented(c.H, c.strand), c.V, rec["tbegH"], rec["tendH"], rec["tbegV"], rec["tendV"])
            assert got == {f: rec[f] for f in got}, (c.name, b0)
            assert rec["band"] == max(s[-1][0] for s in steps) and rec["widened"] == sum(1 for s in steps for a, b in zip(s, s[1:]) if b[0] == 2 * a[0])
            assert len(steps[0]) == len(steps[1])
            merged += len(ops) == 1
    assert merged >= 2 * len(T.BAND0S)                                   # seam_equal_*: one '=' run through both seams
    seams = {c.name: M.cigar(expect[0][q][1]) for q, c in enumerate(cases) if c.name.startswith("seam")}
    assert seams["seam_xx_both_0"] == "179=2X7=1X7=2X209=" and seams["seam_all_x_0"] == "180=17X210=", seams

