"""CPU tests of the read correction: the numpy mirror against hand-written tables, the consensus rule at its
boundaries, the edit distance, the ABI additions and the command line's --correct rules.  No device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bella_amd import _lib, api
from bella_testkit import pileup_mirror as P
from bella_testkit import trace_mirror as M
from conftest import ROOT

A, C, G, T, DEL, IA, IC, IG, IT = range(9)


def _table(n, entries):
    """(n, 9) table from {position: {counter: votes}}"""
    t = np.zeros((n, 9), np.uint32)
    for p, row in entries.items():
        for c, v in row.items():
            t[p, c] = v
    return t


def _pair_tables(cigar, H, V, strand, tbegH=0, tbegV=0):
    """tables of V and of H (own strand) from one traced pair, through P.pileup"""
    ops = M.parse_cigar(cigar)
    pairs = np.zeros(1, _lib.PAIR_DT)
    alns = np.zeros(1, _lib.ALN_DT)
    tr = np.zeros(1, _lib.TRACE_DT)
    pairs[0]["rid"], pairs[0]["cid"] = 1, 0
    alns[0]["strand"] = strand
    tr[0]["nops"], tr[0]["tbegH"], tr[0]["tbegV"] = len(ops), tbegH, tbegV
    table, dropped = P.pileup([V, H], pairs, alns, tr, ops)
    assert table.dtype == np.uint32 and table.shape == (len(V) + len(H), 9)
    return table[:len(V)], table[len(V):], dropped


def test_votes_of_a_pair_with_one_x_one_i_one_d():
    """V  A C G T A - C
       H' A C T T - G C      2= 1X 1= 1I 1D 1="""
    V, Hp = b"ACGTAC", b"ACTTGC"
    M.replay(M.parse_cigar("2=1X1=1I1D1="), Hp, V, 0, 6, 0, 6)
    tv, th, dropped = _pair_tables("2=1X1=1I1D1=", Hp, V, 0)
    want_v = _table(6, {0: {A: 1}, 1: {C: 1}, 2: {T: 1}, 3: {T: 1}, 4: {DEL: 1}, 5: {C: 1, IG: 1}})
    want_h = _table(6, {0: {A: 1}, 1: {C: 1}, 2: {G: 1}, 3: {T: 1}, 4: {DEL: 1, IA: 1}, 5: {C: 1}})
    assert np.array_equal(tv, want_v) and np.array_equal(th, want_h) and dropped == 0
    # the same pair on strand 1: H = revcomp(H').  V's rows are the same; H's counters at mirrored positions, bases complemented,
    # the inserted base in junction lenH - 4 = 2
    H = M.revcomp(Hp)
    assert H == b"GCAAGT"
    tv1, th1, dropped = _pair_tables("2=1X1=1I1D1=", H, V, 1)
    want_h1 = _table(6, {5: {T: 1}, 4: {G: 1}, 3: {C: 1}, 2: {A: 1, IT: 1}, 1: {DEL: 1}, 0: {G: 1}})
    assert np.array_equal(tv1, want_v) and np.array_equal(th1, want_h1) and dropped == 0


def test_a_run_of_inserted_bases_is_one_vote():
    """a two-base D run: V gets ONE ins vote, with the run's first base; H' two del votes.  A two-base I run on both strands: H gets
    one vote -- strand 0 the run's first base, strand 1 the complement of its LAST base (the first in H's own direction)"""
    V, Hp = b"ACGT", b"ACTGGT"
    M.replay(M.parse_cigar("2=2D2="), Hp, V, 0, 6, 0, 4)
    tv, th, _ = _pair_tables("2=2D2=", Hp, V, 0)
    assert np.array_equal(tv, _table(4, {0: {A: 1}, 1: {C: 1}, 2: {G: 1, IT: 1}, 3: {T: 1}}))
    assert np.array_equal(th, _table(6, {0: {A: 1}, 1: {C: 1}, 2: {DEL: 1}, 3: {DEL: 1}, 4: {G: 1}, 5: {T: 1}}))
    V, Hp = b"ACGTCA", b"ACCA"
    M.replay(M.parse_cigar("2=2I2="), Hp, V, 0, 4, 0, 6)
    want_v = _table(6, {0: {A: 1}, 1: {C: 1}, 2: {DEL: 1}, 3: {DEL: 1}, 4: {C: 1}, 5: {A: 1}})
    tv, th, _ = _pair_tables("2=2I2=", Hp, V, 0)
    assert np.array_equal(tv, want_v)
    assert np.array_equal(th, _table(4, {0: {A: 1}, 1: {C: 1}, 2: {C: 1, IG: 1}, 3: {A: 1}}))
    H = M.revcomp(Hp)
    assert H == b"TGGT"
    tv, th, _ = _pair_tables("2=2I2=", H, V, 1)
    assert np.array_equal(tv, want_v)
    # H' 0..3 = H 3..0; the run G T sits in junction 2 of H' = junction 4 - 2 = 2 of H; H's direction meets T first: complement A
    assert np.array_equal(th, _table(4, {3: {T: 1}, 2: {G: 1, IA: 1}, 1: {G: 1}, 0: {T: 1}}))


def test_votes_for_the_junction_behind_the_last_base_are_dropped():
    tv, th, dropped = _pair_tables("2=2I", b"AC", b"ACGT", 0)                  # I run at j = lenH
    assert dropped == 1 and int(th.sum()) == 2 and np.array_equal(tv, _table(4, {0: {A: 1}, 1: {C: 1}, 2: {DEL: 1}, 3: {DEL: 1}}))
    tv, th, dropped = _pair_tables("2=2D", b"ACGT", b"AC", 0)                  # D run at i = lenV
    assert dropped == 1 and int(tv.sum()) == 2 and np.array_equal(th, _table(4, {0: {A: 1}, 1: {C: 1}, 2: {DEL: 1}, 3: {DEL: 1}}))
    tv, th, dropped = _pair_tables("2I2=", M.revcomp(b"AC"), b"GTAC", 1)       # strand 1: junction 0 of H' is junction lenH of H
    assert dropped == 1 and np.array_equal(th, _table(2, {1: {T: 1}, 0: {G: 1}})) and int(tv[:, DEL].sum()) == 2
    # an offset start: the ops begin at (tbegV, tbegH)
    tv, th, dropped = _pair_tables("2=", b"TTAC", b"GAC", 0, tbegH=2, tbegV=1)
    assert dropped == 0 and np.array_equal(tv, _table(3, {1: {A: 1}, 2: {C: 1}})) and np.array_equal(th, _table(4, {2: {A: 1}, 3: {C: 1}}))


def test_votes_accumulate_over_pairs_and_both_roles():
    """two pairs on three reads: read 1 is H of the first and V of the second"""
    reads = [b"ACGT", b"ACTT", b"ACGT"]
    pairs = np.zeros(2, _lib.PAIR_DT)
    alns = np.zeros(2, _lib.ALN_DT)
    tr = np.zeros(3, _lib.TRACE_DT)[:2]
    pairs["rid"], pairs["cid"] = [1, 2], [0, 1]
    ops = np.concatenate([M.parse_cigar("2=1X1="), M.parse_cigar("2=1X1=")])
    tr["nops"], tr["op_off"] = [3, 3], [0, 3]
    table, dropped = P.pileup(reads, pairs, alns, tr, ops)
    want = np.concatenate([_table(4, {0: {A: 1}, 1: {C: 1}, 2: {T: 1}, 3: {T: 1}}), _table(4, {0: {A: 2}, 1: {C: 2}, 2: {G: 2}, 3: {T: 2}}),
                           _table(4, {0: {A: 1}, 1: {C: 1}, 2: {T: 1}, 3: {T: 1}})])
    assert np.array_equal(table, want) and dropped == 0
    tr["nops"][1] = 0                                                          # an untraced pair does not vote
    table, _ = P.pileup(reads, pairs, alns, tr, ops)
    assert int(table[8:].sum()) == 0 and int(table[4:8].sum()) == 4


def test_consensus_rule_at_its_boundaries():
    # ties: the own base wins when it is among the maxima (C: 2 + 1 own = A: 3), else the smallest code (own T: A 2, C 2, T 0 + 1)
    seq, st = P.consensus(b"CT", _table(2, {0: {A: 3, C: 2}, 1: {A: 2, C: 2}}), 3)
    assert seq == b"CA" and st == dict(len_before=2, len_after=2, substituted=1, deleted=0, inserted=0, covered=2, depth_sum=9)
    # min_depth: depth 2 keeps the own base whatever the votes say, depth 3 follows them
    seq, st = P.consensus(b"TT", _table(2, {0: {A: 2}, 1: {A: 3}}), 3)
    assert seq == b"TA" and st["covered"] == 1 and st["substituted"] == 1
    assert P.consensus(b"TT", _table(2, {0: {A: 2}, 1: {A: 3}}), 2)[0] == b"AA"
    assert P.consensus(b"TT", _table(2, {0: {A: 2}, 1: {A: 3}}), 4)[0] == b"TT"
    # deletion: 2 del > depth + 1.  depth 5 with del 3: 6 > 6 is false, the base stays; depth 6 with del 4: 8 > 7, it goes
    seq, st = P.consensus(b"GG", _table(2, {0: {G: 2, DEL: 3}, 1: {G: 2, DEL: 4}}), 3)
    assert seq == b"G" and st["deleted"] == 1 and st["len_after"] == 1 and st["depth_sum"] == 11
    # insertion: c = min(depth(p-1), depth(p)), 2 I > c + 1.  c = 5 with I = 3: 6 > 6 is false; I = 4: 8 > 6; ties to the smallest code
    five = {G: 5}
    assert P.consensus(b"GG", _table(2, {0: five, 1: {G: 5, IA: 1, IT: 2}}), 3)[0] == b"GG"
    seq, st = P.consensus(b"GG", _table(2, {0: five, 1: {G: 5, IC: 2, IT: 2}}), 3)
    assert seq == b"GCG" and st["inserted"] == 1 and st["len_after"] == 3
    # c is the SMALLER depth: the left neighbour has depth 2 < min_depth, no insertion; and the junction before position 0 never emits
    assert P.consensus(b"GG", _table(2, {0: {G: 2}, 1: {G: 5, IC: 4}}), 3)[0] == b"GG"
    assert P.consensus(b"GG", _table(2, {0: {G: 5, IC: 9}, 1: five}), 3)[0] == b"GG"
    # a deleted position and an inserted junction side by side; an untouched read comes back as it is
    seq, st = P.consensus(b"ACGT", _table(4, {0: {A: 4}, 1: {C: 4}, 2: {DEL: 4, IT: 4}, 3: {T: 4}}), 3)
    assert seq == b"ACTT" and st["deleted"] == 1 and st["inserted"] == 1 and st["substituted"] == 0
    seq, st = P.consensus(b"ACGT", np.zeros((4, 9), np.uint32), 1)
    assert seq == b"ACGT" and st == dict(len_before=4, len_after=4, substituted=0, deleted=0, inserted=0, covered=0, depth_sum=0)
    assert P.consensus(b"", np.zeros((0, 9), np.uint32), 3)[0] == b""


def test_edit_distance_against_the_scalar_recurrence():
    def brute(a, b):
        D = list(range(len(b) + 1))
        for i in range(1, len(a) + 1):
            E = [i] + [0] * len(b)
            for j in range(1, len(b) + 1):
                E[j] = min(D[j - 1] + (a[i - 1] != b[j - 1]), D[j] + 1, E[j - 1] + 1)
            D = E
        return D[len(b)]
    rng = np.random.default_rng(6)
    cases = [(b"", b""), (b"ACGT", b""), (b"", b"ACGT"), (b"ACGT", b"ACGT"), (b"AAAA", b"CCCC"), (b"ACGT", b"AGT"), (b"kitten", b"sitting")]
    for _ in range(100):
        cases.append(tuple(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(0, 40))).tolist()) for _ in range(2)))
    for a, b in cases:
        assert P.edit_distance(a, b) == brute(a, b), (a, b)


def test_pileup_structs_and_symbols_as_a_c_compiler_sees_them(tmp_path):
    """the new entry points exist, the ABI version stays 6, bella_memory keeps its size, and bella_consensus_params /
    bella_consensus_read / the grown bella_trace_stats have the layout of the ctypes / numpy mirrors"""
    lib = _lib.load()
    assert lib.bella_hip_abi_version() == 6
    for name in ("bella_hip_pileup_reset", "bella_hip_trace_pairs_pileup", "bella_hip_get_pileup", "bella_hip_add_pileup", "bella_hip_get_pileup_bytes",
                 "bella_hip_consensus", "bella_hip_get_consensus", "bella_hip_write_fasta"):
        assert hasattr(lib, name), name
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {',
           'printf("bella_memory size %zu\\n", sizeof(bella_memory));', 'printf("bella_consensus_params size %zu\\n", sizeof(bella_consensus_params));',
           'printf("bella_consensus_read size %zu\\n", sizeof(bella_consensus_read));', 'printf("bella_trace_stats size %zu\\n", sizeof(bella_trace_stats));',
           'printf("pileup counters %d\\n", BELLA_PILEUP_COUNTERS);']
    for f, _ in _lib.ConsensusParams._fields_:
        src.append('printf("bella_consensus_params %s %%zu\\n", offsetof(bella_consensus_params, %s));' % (f, f))
    for f in _lib.CONS_DT.names:
        src.append('printf("bella_consensus_read %s %%zu\\n", offsetof(bella_consensus_read, %s));' % (f, f))
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
    assert got[("bella_memory", "size")] == ctypes.sizeof(_lib.Memory) == 80
    assert got[("bella_consensus_params", "size")] == ctypes.sizeof(_lib.ConsensusParams) == 8
    assert got[("bella_consensus_read", "size")] == _lib.CONS_DT.itemsize == 32
    assert got[("bella_trace_stats", "size")] == ctypes.sizeof(_lib.TraceStats) == 120
    assert got[("pileup", "counters")] == _lib.PILEUP_COUNTERS == P.NCOUNTERS == 9
    for f, _ in _lib.ConsensusParams._fields_:
        assert got[("bella_consensus_params", f)] == getattr(_lib.ConsensusParams, f).offset, f
    for f in _lib.CONS_DT.names:
        assert got[("bella_consensus_read", f)] == _lib.CONS_DT.fields[f][1], f
    for f, _ in _lib.TraceStats._fields_:
        assert got[("bella_trace_stats", f)] == getattr(_lib.TraceStats, f).offset, f
    assert [f for f, _ in _lib.TraceStats._fields_][-3:] == ["vote_ms", "votes", "ops_host_bytes"]


def test_write_fasta_is_plain_host_code(tmp_path):
    f = str(tmp_path / "c.fasta")
    offs = np.array([0, 4, 4, 7], np.uint64)
    api.write_fasta(f, ["a", "empty", "c"], offs, np.frombuffer(b"ACGTTTT", np.uint8))
    assert open(f, "rb").read() == b">a\nACGT\n>empty\n\n>c\nTTT\n"
    api.write_fasta(f, ["d"], np.array([0, 2], np.uint64), np.frombuffer(b"GG", np.uint8), append=True)
    assert open(f, "rb").read() == b">a\nACGT\n>empty\n\n>c\nTTT\n>d\nGG\n"
    api.write_fasta(f, ["d"], np.array([0, 2], np.uint64), np.frombuffer(b"GG", np.uint8))
    assert open(f, "rb").read() == b">d\nGG\n"
    with pytest.raises(api.BellaHipError):
        api.write_fasta(str(tmp_path / "no" / "dir.fasta"), ["d"], np.array([0, 2], np.uint64), np.frombuffer(b"GG", np.uint8))


def test_cli_correct_rules_without_a_device(tmp_path):
    from bella_amd import build as b
    exe = b.build_cli()
    run = lambda args: subprocess.run([exe] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    p = run(["--help"])
    assert p.returncode == 0 and b"--correct" in p.stdout and b"--min-depth" in p.stdout and b"--cigar" in p.stdout and b"--trace-band" in p.stdout
    for bad, msg in ((["--correct", "c.fa", "--skip-alignment"], b"--correct"), (["--correct", "c.fa", "--min-depth", "0"], b"--min-depth"),
                     (["--correct", "c.fa", "--min-depth", "-2"], b"--min-depth"), (["--min-depth", "4"], b"--correct"), (["--correct"], b"missing an argument"),
                     (["--correct", "c.fa", "--trace-band", "-4"], b"--trace-band"), (["--correct", "c.fa", "--cigar"], b"--cigar")):
        p = run(["-f", "in.txt", "-o", "x"] + bad)
        assert p.returncode == 1 and b"bella-hip:" in p.stderr and msg in p.stderr, (bad, p.stderr)
    # accepted combinations get as far as the list file (which is not there)
    for ok in (["--correct", "c.fa"], ["--correct", "c.fa", "--min-depth", "1"], ["--correct", "c.fa", "--trace-band", "512"],
               ["--correct", "c.fa", "--paf", "--cigar"], ["--correct=c.fa", "--paf"]):
        p = run(["-f", "missing.txt", "-o", "x"] + ok)
        assert p.returncode == 1 and b"Could not open missing.txt" in p.stderr, (ok, p.stderr)
