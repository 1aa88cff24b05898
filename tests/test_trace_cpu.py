"""CPU tests of the traced alignments: the numpy mirror against a scalar DP, the replay checker, the true-PAF
writer (plain host code), the command line's --cigar rules and the ABI additions.  No device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bella_amd import _lib, api
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
