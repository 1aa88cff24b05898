"""CPU tests of the unitig consensus, mirror only: unitig_mirror.polished against an independent brute-force
statement built on pileup_mirror.consensus, on tables that take every branch of the rule; the three facts that follow from the
definition; the GFA / FASTA text with polished arrays; the command line's refusals."""
import subprocess

import numpy as np
import pytest

from bella_testkit import pileup_mirror as P
from bella_testkit import unitig_mirror as U


@pytest.fixture(scope="module")
def cases():
    out = []
    for name, seqs, recs, graph, clean in U.polish_cases():
        m, c, u = U.case_unitigs(seqs, recs, graph, clean)
        out.append((name, seqs, u))
    return out


def _brute(u, seqs, table, min_depth):
    """the definition by way of whole-read consensus calls: the decisions of the positions [a, b) of a read are what
    consensus(read[:b]) has behind consensus(read[:a]) -- a decision reads its own row and the row before it, nothing else"""
    lens = np.array([len(s) for s in seqs], np.int64)
    roff = np.concatenate([[0], np.cumsum(lens)])
    voff = u["voff"].astype(np.int64).tolist()
    offs, segs, pos, nb = [0], [], [], []
    for k in range(len(u["len"])):
        at = 0
        for v, n in zip(u["verts"][voff[k]:voff[k + 1]].tolist(), u["nbases"][voff[k]:voff[k + 1]].tolist()):
            r, L = v >> 1, int(lens[v >> 1])
            rows = table[roff[r]:roff[r + 1]]
            a, b = (L - n, L) if v & 1 else (0, n)
            whole, _ = P.consensus(seqs[r][:b], rows[:b], min_depth)
            head, _ = P.consensus(seqs[r][:a], rows[:a], min_depth)
            assert whole[:len(head)] == head
            seg = whole[len(head):]
            seg = U.revcomp(seg) if v & 1 else seg
            segs.append(seg); pos.append(at); nb.append(len(seg))
            at += len(seg)
        offs.append(offs[-1] + at)
    return offs, b"".join(segs), pos, nb


def test_random_tables_take_every_branch(cases):
    name, seqs, u = cases[0]
    lens = [len(s) for s in seqs]
    for seed in range(3):
        t = U.random_table(lens, seed)
        assert t.dtype == np.uint32 and t.shape == (sum(lens), 9)
        assert np.array_equal(t, U.random_table(lens, seed))
        bc = U.branch_counts(seqs, t, 3)
        print("BRANCHES seed %d: %s" % (seed, bc))
        assert set(bc) == set(U.BRANCHES) and all(bc[k] > 0 for k in U.BRANCHES), bc


@pytest.mark.parametrize("min_depth", [1, 3, 50])
def test_polished_equals_the_brute_force_statement(cases, min_depth):
    seen_rc = False
    for name, seqs, u in cases:
        lens = [len(s) for s in seqs]
        t = U.random_table(lens, 1)
        p = U.polished(u, seqs, t, min_depth)
        offs, bases, pos, nb = _brute(u, seqs, t, min_depth)
        assert p["offsets"].tolist() == offs and p["bases"] == bases and p["pos"].tolist() == pos and p["nbases"].tolist() == nb, name
        assert p["len"].tolist() == np.diff(offs).tolist() and np.array_equal(p["stats"]["len_after"], p["len"])
        assert np.array_equal(p["stats"]["len_before"], u["len"])
        st = p["stats"]
        assert np.array_equal(st["len_after"].astype(np.int64), st["len_before"].astype(np.int64) - st["deleted"].astype(np.int64) + st["inserted"].astype(np.int64))
        assert p["bases"] != U.unitig_bases(u, seqs)[1]
        seen_rc |= bool((u["verts"] & 1).any())
    assert seen_rc


def test_an_all_zero_table_gives_the_raw_unitigs(cases):
    for name, seqs, u in cases:
        t = np.zeros((sum(len(s) for s in seqs), 9), np.uint32)
        p = U.polished(u, seqs, t, 3)
        offs, bases = U.unitig_bases(u, seqs)
        assert np.array_equal(p["offsets"], offs) and p["bases"] == bases and np.array_equal(p["pos"], u["pos"]) and np.array_equal(p["nbases"], u["nbases"]), name
        assert np.array_equal(p["len"], u["len"]) and not p["stats"]["covered"].any() and not p["stats"]["depth_sum"].any()


def test_one_vertex_unitigs_are_the_reads_consensus():
    """orientation 0: the read's consensus; orientation 1: its reverse complement -- with the statistics of bella_consensus_read"""
    rng = np.random.default_rng(9)
    seqs = [U.random_genome(n, 60 + i) for i, n in enumerate((1, 2, 17, 500, 4096))]
    lens = np.array([len(s) for s in seqs])
    roff = np.concatenate([[0], np.cumsum(lens)])
    for seed in range(3):
        t = U.random_table(lens, seed)
        for md in (1, 3):
            for o in (0, 1):
                n = len(seqs)
                u = dict(voff=np.arange(n + 1).astype(np.uint64), verts=(2 * np.arange(n) + o).astype(np.uint32), pos=np.zeros(n, np.uint64), nbases=lens.astype(np.uint32),
                         len=lens.astype(np.uint64), circular=np.zeros(n, np.uint8))
                p = U.polished(u, seqs, t, md)
                for r in range(n):
                    want, st = P.consensus(seqs[r], t[roff[r]:roff[r + 1]], md)
                    got = p["bases"][int(p["offsets"][r]):int(p["offsets"][r + 1])]
                    assert got == (U.revcomp(want) if o else want), (seed, md, o, r)
                    assert {k: int(p["stats"][r][k]) for k in st} == st


def test_window_distance():
    g = U.random_genome(300, 3)
    assert U.window_distance(g[:100], g) == 0 and U.window_distance(g[:100], g[:100]) == 0
    assert U.window_distance(g[:100], g[:90]) == 10 and U.window_distance(b"", g) == 0
    w = g[:40] + b"A" + g[40:100]                                    # one inserted base
    assert U.window_distance(w, g) == 1
    w = g[:40] + g[45:100]                                            # five deleted ones
    assert U.window_distance(w, g) == 5
    for a, b in ((g[:60], g[7:80]), (g[100:160], g[90:200])):
        assert U.window_distance(a, b) == min(P.edit_distance(a, b[:k]) for k in range(len(b) + 1))


def test_gfa_and_fasta_text_with_polished_arrays(cases):
    name, seqs, u = cases[1]                                          # the tip input unclipped: three unitigs, four links
    names = ["r%d" % i for i in range(len(seqs))]
    t = U.random_table([len(s) for s in seqs], 2)
    p = U.polished(u, seqs, t, 3)
    q = U.polished_unitigs(u, p)
    gfa = U.unitig_gfa_text(names, q, p["offsets"], p["bases"])
    raw = U.unitig_gfa_text(names, u, *U.unitig_bases(u, seqs))
    lines, raw_lines = gfa.split(b"\n"), raw.split(b"\n")
    assert len(lines) == len(raw_lines) and len(u["len"]) == 3
    assert [l for l in lines if l.startswith(b"L")] == [l for l in raw_lines if l.startswith(b"L")]      # the links keep their raw overlaps
    S = [l.split(b"\t") for l in lines if l.startswith(b"S")]
    for k, f in enumerate(S):
        assert f[2] == p["bases"][int(p["offsets"][k]):int(p["offsets"][k + 1])] and f[3] == b"LN:i:%d" % len(f[2]) and len(f[2]) == int(p["len"][k])
        assert f[4] == [x for x in raw_lines if x.startswith(b"S")][k].split(b"\t")[4]                  # RC:i: unchanged
    A = [l.split(b"\t") for l in lines if l.startswith(b"a")]
    assert [int(f[2]) for f in A] == p["pos"].tolist() and [int(f[5]) for f in A] == p["nbases"].tolist()
    fa = U.fasta_text(q, p["offsets"], p["bases"])
    assert fa == b"".join(b">%s\n%s\n" % (n.encode(), f[2]) for n, f in zip(U.unitig_names(u), S))


def test_native_cli_refuses_polish_without_its_partners(tmp_path):
    """--polish needs --unitigs or --unitigs-fasta; --polish-min-depth needs --polish; --polish with --gfa-no-seq and no
    --unitigs-fasta has nothing to polish into.  No device is needed: the options are checked before anything runs."""
    from bella_amd import build as b
    exe = b.build_cli()
    run = lambda args: subprocess.run([exe, "-f", "in.txt", "-o", "x"] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    for bad, msg in ((["--polish"], b"--polish needs --unitigs or --unitigs-fasta"),
                     (["--polish", "--gfa", "g.gfa"], b"--polish needs --unitigs or --unitigs-fasta"),
                     (["--unitigs", "u.gfa", "--polish-min-depth", "2"], b"--polish-min-depth needs --polish"),
                     (["--unitigs", "u.gfa", "--polish", "--gfa-no-seq"], b"needs --unitigs-fasta"),
                     (["--unitigs", "u.gfa", "--polish", "--polish-min-depth", "0"], b"at least 1"),
                     (["--unitigs", "u.gfa", "--polish=1"], b"takes no value")):
        p = run(bad)
        assert p.returncode == 1 and b"bella-hip:" in p.stderr and msg in p.stderr, (bad, p.stderr)
    p = run(["--help"])
    assert p.returncode == 0 and b"--polish " in p.stdout and b"--polish-min-depth" in p.stdout
