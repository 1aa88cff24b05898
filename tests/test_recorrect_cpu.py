"""Read correction rounds without a device: the job frames by hand, the anchors and their composition, the mirror
alone on a small genome, the new structs as a C compiler sees them, the command line's argument errors."""
import ctypes
import os
import subprocess

import numpy as np

from bella_amd import _lib
from bella_testkit import graph_mirror as G
from bella_testkit import pileup_mirror as P
from bella_testkit import recorrect_cases as RC
from bella_testkit import recorrect_mirror as M
from bella_testkit import trace_mirror as T
from bella_testkit import unitig_mirror as U
from conftest import ROOT


def _noisy(template: bytes, rng, err=0.15, mix=(0.10, 0.60, 0.30)):
    """a read of `template` at the generator's error mix: (read, cum) with cum[t] = bases of the read in front of template base t"""
    out, cum = [], [0]
    p_sub, p_ins, p_del = (err * m for m in mix)
    for ch in template:
        x = rng.random()
        if x >= p_del:
            out.append(b"ACGT"[(b"ACGT".index(ch) + rng.integers(1, 4)) & 3] if x < p_del + p_sub else ch)
            if p_del + p_sub <= x < p_del + p_sub + p_ins:
                out.append(b"ACGT"[rng.integers(0, 4)])
        cum.append(len(out))
    return bytes(out), cum


def _zero_round1(seqs):
    return M.first_round(seqs, np.zeros((sum(map(len, seqs)), 9), np.uint32), 3)


def test_the_four_frames_by_hand():
    """L_H = 100, strand 1, begH = 10, endH = 70 (the docstring's numbers); then error-free reads cut from one genome: [s, e) is the true
    position and every job is free of X, I and D"""
    rec = np.array([(0, 1, 5, 65, 10, 70, 0, 1, (0, 0, 0)), (0, 1, 5, 65, 10, 70, 0, 0, (0, 0, 0))], G.OVL_DT)
    J, W = M.jobs(rec, [80, 100])
    assert [(int(j["target"]), int(j["query"]), int(j["orient"]), int(j["qbeg"]), int(j["qend"])) for j in J] == [(0, 1, 1, 30, 90), (1, 0, 1, 5, 65), (0, 1, 0, 10, 70), (1, 0, 0, 5, 65)]
    assert W.tolist() == [[5, 65], [30, 90], [5, 65], [10, 70]]
    genome = U.random_genome(3000, 7)
    starts, lens, strands = [0, 400, 900, 1300, 1500], [1200, 1300, 1000, 1500, 700], [0, 1, 1, 0, 0]
    seqs = U.reads_from_genome(genome, starts, lens, strands)
    recs = G.truth_records(starts, lens, strands, min_overlap=100)
    seen = set()
    m = M.recorrect_round(_zero_round1(seqs), seqs, recs, band0=256)
    for j, w in zip(m["jobs"], M.jobs(recs, lens)[1]):
        assert (int(j["s"]), int(j["e"])) == (int(w[0]), int(w[1])) == (int(j["q_begin"]), int(j["q_end"])), j
        assert int(j["status"]) == M.VOTED and int(j["n_x"]) == int(j["n_ins"]) == int(j["n_del"]) == 0 and int(j["n_eq"]) == int(j["qend"]) - int(j["qbeg"])
        seen.add((int(j["side"]), int(j["orient"])))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)} and m["bases"] == b"".join(seqs)


def test_the_coordinate_map_and_its_composition():
    """P is exact at every anchor, monotone, P(L) = plen; the anchors of two rounds equal those of the per-base composition"""
    rng = np.random.default_rng(3)
    for L in (0, 1, 255, 256, 257, 512, 1000):
        e1 = rng.integers(0, 3, L)                                    # emitted per raw base
        a1 = M.anchors(e1)
        scan1 = np.concatenate([[0], np.cumsum(e1)])
        plen = int(scan1[-1])
        assert len(a1) == M.nanchors(L) and int(a1[-1]) == plen
        p = [M.to_corrected(x, L, a1, plen) for x in range(L + 1)]
        assert all(p[x] == scan1[x] for x in range(0, L + 1, M.STEP)) and p[L] == plen and all(x <= y for x, y in zip(p, p[1:]))
        e2 = rng.integers(0, 3, plen)                                 # the second round decides on the first one's sequence
        a2 = M.anchors(e2, a1)
        scan2 = np.concatenate([[0], np.cumsum(e2)])
        direct = [int(scan2[scan1[min(M.STEP * j, L)]]) for j in range(M.nanchors(L))]
        assert a2.tolist() == direct and int(a2[-1]) == int(scan2[-1])


def test_two_rounds_correct_reads_built_from_truth():
    """A 6 kb genome, 40 reads of 1.5 kb at the generator's mix (15 % error): 10 x, so that two numpy DPs per record stay within a
    minute.  Records from truth: every pair that shares 500 template bases, an extension anchored at the true start of the overlap
    (tests/test_realign_cpu.py's layout); round 1 is the consensus of the pileup of those extensions.  The summed global distance of all
    40 reads to their templates (60,000 template bases), measured: raw 8,444 (14.07 %), round 1 2,653 (4.42 %), round 2 1,343 (2.24 %),
    round 3 1,278 (2.13 %); 297 records, all 594 jobs of round 2 voted.  Condition: round 2 is BELOW round 1."""
    rng = np.random.default_rng(77)
    glen, L = 6000, 1500
    genome = U.random_genome(glen, 78)
    n = 10 * glen // L
    starts = np.sort(np.concatenate([[0, glen - L], rng.integers(0, glen - L + 1, n - 2)]))
    strands = rng.integers(0, 2, n)
    fwd, cums = zip(*(_noisy(genome[s:s + L], rng) for s in starts.tolist()))
    seqs = [T.revcomp(f) if o else f for f, o in zip(fwd, strands.tolist())]
    pairs, alns, traces, ops, recs = [], [], [], [], []
    for v in range(n):
        for h in range(v + 1, n):
            lo, hi = max(starts[v], starts[h]), min(starts[v], starts[h]) + L
            if hi - lo < 500:
                continue
            if strands[v] == 0:
                tv, th = cums[v][lo - starts[v]], cums[h][lo - starts[h]]
            else:
                tv, th = len(fwd[v]) - cums[v][hi - starts[v]], len(fwd[h]) - cums[h][hi - starts[h]]
            st = int(strands[v] ^ strands[h])
            Hp = T.oriented(seqs[h], st)
            score, (i, j), o, _ = T.banded_extension(Hp[th:], seqs[v][tv:], 256)
            runs = T.run_lengths(o[::-1])
            pairs.append((h, v)); alns.append(st); traces.append((len(runs), sum(len(q) for q in ops), tv, th))
            ops.append(runs)
            recs.append((v, h, tv, tv + i, th, th + j, score, st, (0, 0, 0)))
    pairs = np.array(pairs, [("rid", "<u4"), ("cid", "<u4")])
    alns = np.array(alns, [("strand", "<u4")])
    traces = np.array(traces, [("nops", "<u4"), ("op_off", "<u8"), ("tbegV", "<i4"), ("tbegH", "<i4")])
    table, _ = P.pileup(seqs, pairs, alns, traces, np.concatenate(ops))
    recs = np.array(recs, G.OVL_DT)
    rounds = [M.first_round(seqs, table, 3)]
    for _ in range(2):
        rounds.append(M.recorrect_round(rounds[-1], seqs, recs, band0=256))

    def total(bases, offs):
        d = 0
        for r in range(n):
            t = genome[starts[r]:starts[r] + L]
            d += P.edit_distance(bases[int(offs[r]):int(offs[r + 1])], T.revcomp(t) if strands[r] else t)
        return d
    roff = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    d = [total(b"".join(seqs), roff)] + [total(x["bases"], x["offsets"]) for x in rounds]
    print("RECORRECT mirror, 6 kb genome, %d reads of 1.5 kb at 15 %%, %d records: distance to the templates raw %d, round 1 %d, round 2 %d, round 3 %d; round 2 %s"
          % (n, len(recs), d[0], d[1], d[2], d[3], rounds[1]["counts"]))
    assert d[2] < d[1], d


def test_the_mixed_case_covers_what_the_gpu_tests_need():
    seqs, recs = RC.mixed_case()
    cur = M.first_round(seqs, RC.mixed_table(seqs), 3)
    assert len(seqs[RC.SHORT]) < M.STEP and len(seqs[RC.TWO_STEPS]) == 2 * M.STEP and int(cur["offsets"][RC.EMPTY + 1] - cur["offsets"][RC.EMPTY]) == 0
    a = M.recorrect_round(cur, seqs, recs, band0=256, band_max=2048)["jobs"]
    assert ((a["status"] == M.VOTED) & (a["band"] == 512)).any() and (a["status"] == M.LOW_IDENTITY).any() and ((a["status"] == M.NONE) & (a["target"] == RC.EMPTY)).sum() == 1
    b = M.recorrect_round(cur, seqs, recs, band0=512, band_max=512)
    assert (b["jobs"]["status"] == M.BAND_CAPPED).any()
    r = RC.NO_RECORD
    assert b["bases"][int(b["offsets"][r]):int(b["offsets"][r + 1])] == seqs[r]


def test_recorrect_structs_equal_the_header_as_a_c_compiler_sees_them(tmp_path):
    structs = {"bella_recorrect_params": _lib.RecorrectParams, "bella_recorrect_stats": _lib.RecorrectStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            src.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    src.append('printf("bella_recorrect_job size %zu\\n", sizeof(bella_recorrect_job));')
    for fname in _lib.RECJOB_DT.names:
        src.append('printf("bella_recorrect_job %s %%zu\\n", offsetof(bella_recorrect_job, %s));' % (fname, fname))
    src.append('printf("bella_consensus_read size %zu\\n", sizeof(bella_consensus_read));')
    src.append('printf("abi version %d\\n", BELLA_HIP_ABI_VERSION);')
    src.append('printf("anchor step %d\\n", BELLA_RECORRECT_ANCHOR_STEP);')
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    protos = tmp_path / "protos.c"                                    # the prototypes, as a C compiler reads them (compiled, not linked)
    protos.write_text('#include "bella_hip.h"\n'
                      'int (*run)(bella_ctx*, const bella_recorrect_params*, uint64_t*) = bella_hip_recorrect;\n'
                      'int (*get)(bella_ctx*, uint64_t*, uint8_t*, bella_consensus_read*) = bella_hip_get_recorrected;\n'
                      'int (*jobs)(bella_ctx*, uint64_t*, bella_recorrect_job*) = bella_hip_get_recorrect_jobs;\n'
                      'int (*ops)(bella_ctx*, uint64_t*, uint32_t*, uint32_t*) = bella_hip_get_recorrect_ops;\n'
                      'int (*st)(bella_ctx*, void*, uint64_t) = bella_hip_get_recorrect_stats;\n'
                      'int (*an)(bella_ctx*, uint64_t*, uint64_t*) = bella_hip_get_recorrect_anchors;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert got[("bella_recorrect_job", "size")] == _lib.RECJOB_DT.itemsize == M.JOB_DT.itemsize == 104
    for fname in _lib.RECJOB_DT.names:
        assert got[("bella_recorrect_job", fname)] == _lib.RECJOB_DT.fields[fname][1] == M.JOB_DT.fields[fname][1], fname
    assert ctypes.sizeof(_lib.RecorrectParams) == 24 and ctypes.sizeof(_lib.RecorrectStats) == 152
    assert got[("bella_consensus_read", "size")] == _lib.CONS_DT.itemsize == M.CONS_DT.itemsize == 32
    assert got[("anchor", "step")] == M.STEP == _lib.RECORRECT_ANCHOR_STEP
    # additive: the version stays what it was, and the library exports the entry points
    assert got[("abi", "version")] == 6 and _lib.load().bella_hip_abi_version() == 6
    for name in ("bella_hip_recorrect", "bella_hip_get_recorrected", "bella_hip_get_recorrect_jobs", "bella_hip_get_recorrect_ops", "bella_hip_get_recorrect_stats"):
        assert hasattr(_lib.load(), name), name


def _cli():
    from bella_amd import build as b
    return b.build_cli()


def test_cli_help_lists_the_options():
    p = subprocess.run([_cli(), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0
    for opt in ("--correct-rounds arg", "--correct-band arg", "--correct-min-identity arg"):
        assert opt in p.stdout.decode(), opt


def test_cli_refuses_the_options_without_correct_and_out_of_range():
    """all of these are decided before a device is looked for"""
    need = "need --correct"
    cor = ["--correct", "c.fasta"]
    for flags, word in ((["--correct-rounds", "2"], need), (["--correct-band", "512"], need), (["--correct-min-identity", "600"], need),
                        (cor + ["--correct-rounds", "0"], "--correct-rounds must be in [1, 4]"),
                        (cor + ["--correct-rounds", "5"], "--correct-rounds must be in [1, 4]"),
                        (cor + ["--correct-band", "300"], "--correct-band must be a power of two"),
                        (cor + ["--correct-band", "128"], "--correct-band must be a power of two"),
                        (cor + ["--correct-band", "8192"], "--correct-band must be a power of two"),
                        (cor + ["--correct-min-identity", "1001"], "--correct-min-identity is in permille")):
        p = subprocess.run([_cli(), "-f", "none.txt", "-o", "none"] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and word in p.stderr.decode(), (flags, p.stderr)
