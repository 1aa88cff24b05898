"""CPU tests of the clipped ends: the numpy mirror's run-level definition against a brute-force search over
columns, the properties of a clipped path, the hand-made cases of the GPU test, the ABI additions and the command line's rules.  No device."""
import ctypes
import os
import subprocess

import numpy as np

from bella_amd import _lib
from bella_testkit import clip_cases as CC
from bella_testkit import clip_mirror as K
from conftest import ROOT

EQ, X, INS, DEL = 0, 1, 2, 3


def _small_random(rng):
    """a short run list with small lengths, so that ties and zero sums are frequent"""
    n = int(rng.integers(0, 13))
    out, prev = [], -1
    for _ in range(n):
        op = int(rng.choice([o for o in (EQ, EQ, X, INS, DEL) if o != prev]))
        out.append(CC.w(rng.integers(1, 5), op))
        prev = op
    return out


def test_run_level_definition_is_the_column_level_one():
    """4,000 random run lists at identities that make ties common (500: +1 / -1; 250 and 750: 3 to 1) and at the default: the mirror's
    (a, b) are the runs of the brute-force column segment, the value is the same, the tie rule included"""
    rng = np.random.default_rng(1)
    emptied = ties = 0
    for n in range(4000):
        words = _small_random(rng)
        t = (500, 250, 750, 650, 1, 999)[n % 6]
        a, b, v = K.segment(words, t)
        want = K.brute_columns(words, t)
        if want is None:
            assert (a, b, v) == (0, 0, 0), (words, t)
            emptied += 1
            continue
        lens = np.asarray(words, np.int64) >> 4
        col = np.concatenate([[0], np.cumsum(lens)])
        assert (int(col[a]), int(col[b]), v) == want, (words, t, (a, b, v), want)
        wt = K.weights(words, t)
        P = np.concatenate([[0], np.cumsum(wt)])
        ties += int(((P[None, 1:] - P[:-1, None]) == v).sum() > 1)
    assert emptied > 100 and ties > 300                       # (not vacuous: both happen often)


def test_properties_of_a_clipped_path():
    rng = np.random.default_rng(2)
    for n in range(600):
        words = np.asarray(CC.random_runs(rng, int(rng.integers(0, 200))), np.uint32)
        t = CC.IDENTITIES[n % 5]
        tv, th = int(rng.integers(0, 500)), int(rng.integers(0, 500))
        r = K.clip_one(words, tv, th, t)
        a, b = int(r["first_run"]), int(r["first_run"]) + int(r["nruns"])
        if r["nruns"] == 0:
            assert (int(r["begV"]), int(r["endV"]), int(r["begH"]), int(r["endH"])) == (tv, tv, th, th)
            assert int(r["n_eq"]) + int(r["n_x"]) + int(r["n_ins"]) + int(r["n_del"]) == 0 and r["score"] == 0 and r["clip_score"] == 0
            continue
        seg = words[a:b]
        assert (seg[0] & 15) == EQ and (seg[-1] & 15) == EQ                      # begins and ends with '='
        assert r["score"] == int(r["n_eq"]) - int(r["n_x"]) - int(r["n_ins"]) - int(r["n_del"])
        assert r["clip_score"] == int(r["n_eq"]) * (1000 - t) - (int(r["n_x"]) + int(r["n_ins"]) + int(r["n_del"])) * t > 0
        assert int(r["endV"]) - int(r["begV"]) == int(r["n_eq"]) + int(r["n_x"]) + int(r["n_ins"])
        assert int(r["endH"]) - int(r["begH"]) == int(r["n_eq"]) + int(r["n_x"]) + int(r["n_del"])
        # idempotence: the clip of the clipped path is the whole of it
        r2 = K.clip_one(seg, int(r["begV"]), int(r["begH"]), t)
        assert r2["first_run"] == 0 and r2["nruns"] == b - a
        for f in ("begV", "endV", "begH", "endH", "n_eq", "n_x", "n_ins", "n_del", "score", "clip_score"):
            assert r2[f] == r[f], f


def test_clip_traces_patches_the_records_and_sums_the_stats():
    rng = np.random.default_rng(3)
    lists = [CC.random_runs(rng, int(rng.integers(0, 40))) for _ in range(50)] + [[], [CC.w(4, X), CC.w(1, INS)], [CC.w(1, EQ), CC.w(1, X)]]
    pairs, ops = CC.build_batch(lists)
    tr = np.zeros(len(pairs), _lib.TRACE_DT)
    for q, words in enumerate(lists):
        w = np.asarray(words, np.int64)
        op, ln = w & 15, w >> 4
        tr[q]["op_off"], tr[q]["nops"], tr[q]["band"], tr[q]["widened"] = pairs[q]["op_off"], len(words), 256, q % 3
        tr[q]["tbegV"], tr[q]["tbegH"] = pairs[q]["tbegV"], pairs[q]["tbegH"]
        tr[q]["tendV"], tr[q]["tendH"] = int(pairs[q]["tbegV"]) + int(ln[op != DEL].sum()), int(pairs[q]["tbegH"]) + int(ln[op != INS].sum())
        for o, f in enumerate(("n_eq", "n_x", "n_ins", "n_del")):
            tr[q][f] = int(ln[op == o].sum())
        tr[q]["score"] = int(tr[q]["n_eq"]) - int(tr[q]["n_x"]) - int(tr[q]["n_ins"]) - int(tr[q]["n_del"])
    out, st = K.clip_traces(tr, ops, 650)
    res, st2 = K.clip_pairs(pairs, ops, 650)
    assert st == st2 and st["pairs"] == sum(1 for x in lists if x) and st["emptied"] > 0 and st["clipped"] > 0
    assert st["runs_after"] == int(out["nops"].sum()) and st["columns_after"] == int(out["n_eq"].sum() + out["n_x"].sum() + out["n_ins"].sum() + out["n_del"].sum())
    assert np.array_equal(out["band"], tr["band"]) and np.array_equal(out["widened"], tr["widened"])
    assert np.array_equal(out["op_off"], tr["op_off"] + res["first_run"]) and np.array_equal(out["nops"], res["nruns"])
    assert np.array_equal(out["tbegV"], res["begV"]) and np.array_equal(out["tendH"], res["endH"]) and np.array_equal(out["score"], res["score"])
    again, st3 = K.clip_traces(out, ops, 650)                 # idempotent on records too
    assert again.tobytes() == out.tobytes() and st3["clipped"] == 0 and st3["emptied"] == 0 and st3["bases_v_removed"] == 0


def test_hand_cases_have_the_segments_they_are_meant_to_have():
    cases = CC.hand_cases()
    assert tuple(len(c[2]) for c in cases[:len(CC.RUN_COUNTS)]) == CC.RUN_COUNTS
    for name, t, words, want in cases:
        a, b, v = K.segment(words, t)
        if want is not None:
            assert (a, b) == want, name
        w = np.asarray(words, np.int64)
        assert int((w >> 4).sum()) < 2 ** 31 - 1000, name      # a pair's bases stay below 2^31
    by = {c[0]: K.segment(c[2], c[1]) for c in cases}
    assert by["in chunk 0"][1] <= 64 and by["in chunk 2"][0] >= 128 and by["chunk 0 into chunk 2"][0] < 64 and by["chunk 0 into chunk 2"][1] > 129
    assert by["2^24 columns"][2] > 2 ** 32


def test_abi_additions(tmp_path):
    lib = _lib.load()
    assert lib.bella_hip_abi_version() == 6
    for name in ("bella_hip_trace_pairs_clip", "bella_hip_clip_ops", "bella_hip_get_clip_stats"):
        assert hasattr(lib, name), name
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {',
           'printf("bella_clip size %zu\\n", sizeof(bella_clip));', 'printf("bella_clip_stats size %zu\\n", sizeof(bella_clip_stats));',
           'printf("bella_clip_params size %zu\\n", sizeof(bella_clip_params));', 'printf("default identity %d\\n", BELLA_CLIP_DEFAULT_IDENTITY);',
           'printf("bella_trace size %zu\\n", sizeof(bella_trace));', 'printf("abi version %d\\n", BELLA_HIP_ABI_VERSION);']
    for f in _lib.CLIP_RES_DT.names:
        src.append('printf("bella_clip %s %%zu\\n", offsetof(bella_clip, %s));' % (f, f))
    for f, _ in _lib.ClipStats._fields_:
        src.append('printf("bella_clip_stats %s %%zu\\n", offsetof(bella_clip_stats, %s));' % (f, f))
    for f, _ in _lib.ClipParams._fields_:
        src.append('printf("bella_clip_params %s %%zu\\n", offsetof(bella_clip_params, %s));' % (f, f))
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    assert got[("bella_clip", "size")] == _lib.CLIP_RES_DT.itemsize == 56
    assert got[("bella_clip_stats", "size")] == ctypes.sizeof(_lib.ClipStats) == 88
    assert got[("bella_clip_params", "size")] == ctypes.sizeof(_lib.ClipParams) == 8
    assert got[("bella_trace", "size")] == _lib.TRACE_DT.itemsize == 56
    assert got[("default", "identity")] == _lib.CLIP_DEFAULT_IDENTITY == K.DEFAULT_IDENTITY == 650 and got[("abi", "version")] == 6
    for f in _lib.CLIP_RES_DT.names:
        assert got[("bella_clip", f)] == _lib.CLIP_RES_DT.fields[f][1], f
    for f, _ in _lib.ClipStats._fields_:
        assert got[("bella_clip_stats", f)] == getattr(_lib.ClipStats, f).offset, f
    for f, _ in _lib.ClipParams._fields_:
        assert got[("bella_clip_params", f)] == getattr(_lib.ClipParams, f).offset, f
    assert [f for f, _ in _lib.ClipStats._fields_] == ["pairs", "clipped", "emptied", "runs_before", "runs_after", "columns_before", "columns_after",
                                                       "bases_v_removed", "bases_h_removed", "identity", "pad", "clip_ms"]
    assert [f for f in _lib.CLIP_RES_DT.names if f != "pad"] == ["first_run", "nruns", "begV", "endV", "begH", "endH", "n_eq", "n_x", "n_ins", "n_del", "score", "clip_score"]


def test_cli_clip_ends_rules(tmp_path):
    from bella_amd import build as b
    exe = b.build_cli()
    run = lambda args: subprocess.run([exe, "-f", "in.txt", "-o", "x"] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    p = run(["--clip-ends"])
    assert p.returncode == 1 and b"bella-hip:" in p.stderr and b"--clip-ends needs an option that traces" in p.stderr, p.stderr
    for o in (b"--cigar", b"--correct", b"--gfa", b"--unitigs", b"--unitigs-fasta", b"--polish"):
        assert o in p.stderr
    p = run(["--clip-identity", "700", "--gfa", "g.gfa"])
    assert p.returncode == 1 and b"--clip-identity needs --clip-ends" in p.stderr
    for bad in ("0", "1000", "-5"):
        p = run(["--clip-ends", "--clip-identity", bad, "--gfa", "g.gfa"])
        assert p.returncode == 1 and b"--clip-identity is in permille: [1, 999]" in p.stderr, (bad, p.stderr)
    p = run(["--clip-ends=1", "--gfa", "g.gfa"])
    assert p.returncode == 1 and b"takes no value" in p.stderr
    open(tmp_path / "in.txt", "w").write("/nonexistent/a.fastq")           # no trailing newline: the rules passed, the list names no file
    for tracing in (["--cigar", "--paf"], ["--correct", "c.fasta"], ["--gfa", "g.gfa"], ["--unitigs", "u.gfa"], ["--unitigs-fasta", "u.fa"],
                    ["--unitigs-fasta", "u.fa", "--polish"]):
        p = run(["--clip-ends", "--clip-identity", "999"] + tracing)
        assert p.returncode == 1 and b"no FASTQ file" in p.stderr, (tracing, p.stderr)
    help_text = run(["--help"]).stdout
    assert b"--clip-ends" in help_text and b"--clip-identity" in help_text
