"""CPU tests of the gap normalisation of the pileup votes: the numpy mirror against hand-worked votes, its four
properties on random alignments, a small simulation of what it buys, the ABI additions and the command line's rule.  No device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from bella_amd import _lib
from bella_testkit import normalize_cases as NC
from bella_testkit import normalize_mirror as N
from bella_testkit import pileup_mirror as P
from bella_testkit import trace_mirror as M
from conftest import ROOT

A, C, G, T, DEL, IA, IC, IG, IT = range(9)
EQ, X, INS, DL = 0, 1, 2, 3


def _table(n, entries):
    t = np.zeros((n, 9), np.int64)
    for p, row in entries.items():
        for c, v in row.items():
            t[p, c] = v
    return t


def _tables(votes_fn, cigar, H, V, strand, tbegH=0, tbegV=0):
    """(table of V, table of H on its own strand, dropped) of one pair"""
    ops = M.parse_cigar(cigar) if isinstance(cigar, str) else np.asarray(cigar, np.uint32)
    tr = dict(op_off=0, nops=len(ops), tbegH=tbegH, tbegV=tbegV)
    res = votes_fn(ops, tr, H, V, strand)
    (pV, cV), (pH, cH), dropped = res[0], res[1], res[2]
    tv, th = np.zeros((len(V), 9), np.int64), np.zeros((len(H), 9), np.int64)
    np.add.at(tv, (pV, cV), 1)
    np.add.at(th, (pH, cH), 1)
    return tv, th, dropped


def _seq_votes(seq):
    """{position: {base: 1}} of a stretch of aligned columns"""
    return {p: {b"ACGT".index(c): 1} for p, c in seq}


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------------------
def test_one_base_insertion_in_a_homopolymer_of_five():
    V, H = b"CGAAAAATC", b"CGAAAATC"                         # 6= 1I 2=: the extra A sits at the right end of the run; sL = 4
    sL, sR = N.shifts(M.parse_cigar("6=1I2="), 0, 0, V, H)
    assert sL.tolist() == [0, 4, 0] and sR.tolist() == [0, 0, 0]
    tv, th, dropped = _tables(N.votes, "6=1I2=", H, V, 0)
    assert dropped == 0
    assert np.array_equal(tv, _table(9, {0: {C: 1}, 1: {G: 1}, 2: {DEL: 1}, 3: {A: 1}, 4: {A: 1}, 5: {A: 1}, 6: {A: 1}, 7: {T: 1}, 8: {C: 1}}))
    assert np.array_equal(th, _table(8, {0: {C: 1}, 1: {G: 1}, 2: {A: 1, IA: 1}, 3: {A: 1}, 4: {A: 1}, 5: {A: 1}, 6: {T: 1}, 7: {C: 1}}))
    pv, ph, _ = _tables(P.votes, "6=1I2=", H, V, 0)            # plain: del at 6, the junction before 6
    assert pv[6, DEL] == 1 and ph[6, IA] == 1 and tv.sum() == pv.sum() and th.sum() == ph.sum()
    # the same indel written at the left end of the run votes the same
    tv2, th2, _ = _tables(N.votes, "2=1I6=", H, V, 0)
    assert np.array_equal(tv, tv2) and np.array_equal(th, th2)


def test_two_base_deletion_in_an_ac_repeat():
    V, H = b"GACACT", b"GACACACT"                            # 5= 2D 1=: S = H', x = 5, L = 2, sL = 4
    sL, sR = N.shifts(M.parse_cigar("5=2D1="), 0, 0, V, H)
    assert sL.tolist() == [0, 4, 0] and sR.tolist() == [0, 0, 0]
    tv, th, dropped = _tables(N.votes, "5=2D1=", H, V, 0)
    assert dropped == 0
    assert np.array_equal(tv, _table(6, {0: {G: 1}, 1: {A: 1, IA: 1}, 2: {C: 1}, 3: {A: 1}, 4: {C: 1}, 5: {T: 1}}))
    assert np.array_equal(th, _table(8, {0: {G: 1}, 1: {DEL: 1}, 2: {DEL: 1}, 3: {A: 1}, 4: {C: 1}, 5: {A: 1}, 6: {C: 1}, 7: {T: 1}}))


def test_gap_behind_a_mismatch_and_gaps_at_the_ends_do_not_shift():
    V, H = b"CGAAAAATC", b"CGAAACTC"                         # 5= 1X 1I 2=
    ops = M.parse_cigar("5=1X1I2=")
    M.replay(ops, H, V, 0, 8, 0, 9)
    assert [a.tolist() for a in N.shifts(ops, 0, 0, V, H)] == [[0, 0, 0, 0], [0, 0, 0, 0]]
    for strand in (0, 1):
        Hs = M.revcomp(H) if strand else H
        n, p = _tables(N.votes, ops, Hs, V, strand), _tables(P.votes, ops, Hs, V, strand)
        assert np.array_equal(n[0], p[0]) and np.array_equal(n[1], p[1]) and n[2] == p[2]
    # first run: nothing before it; last run: nothing behind it -- in a homopolymer where either would slide
    V, H = b"AAAAAAAC", b"AAAAAAAG"                          # 1I 5= 1D from (0, 0)
    ops = M.parse_cigar("1I5=1D")
    sL, sR = N.shifts(ops, 0, 0, V, H)
    assert sL[0] == 0 and sR[2] == 0 and sR[0] == 5 and sL[2] == 5
    tv, th, _ = _tables(N.votes, ops, H, V, 0)                # strand 0: all votes from A_L: run 0 stays, run 2 moves to (1, 0)
    assert tv[0, DEL] == 1 and tv[1, IA] == 1 and th[0, DEL] == 1 and th[0, IA] == 1
    tv1, th1, _ = _tables(N.votes, ops, M.revcomp(H), V, 1)   # strand 1: H from A_R: run 2 stays at j = 5, run 0 moves to (5, 5)
    assert np.array_equal(tv1, tv)
    assert th1[7 - 5, DEL] == 1 and th1[7 - 5 + 1, IT] == 1 and th1[:, DEL].sum() == 1 and th1[:, IA:].sum() == 1


def test_gap_that_uses_its_match_run_up_abuts_another_gap_and_both_vote():
    V, H = b"CGTAAAATC", b"CGAAATC"                          # 2= 1I 3= 1I 2=: the second I slides over all three '=' and lands behind the first
    ops = M.parse_cigar("2=1I3=1I2=")
    M.replay(ops, H, V, 0, 7, 0, 9)
    sL, _ = N.shifts(ops, 0, 0, V, H)
    assert sL.tolist() == [0, 0, 0, 3, 0]
    tv, th, dropped = _tables(N.votes, ops, H, V, 0)
    assert dropped == 0
    assert np.array_equal(tv, _table(9, {0: {C: 1}, 1: {G: 1}, 2: {DEL: 1}, 3: {DEL: 1}, 4: {A: 1}, 5: {A: 1}, 6: {A: 1}, 7: {T: 1}, 8: {C: 1}}))
    assert np.array_equal(th, _table(7, {0: {C: 1}, 1: {G: 1}, 2: {A: 1, IT: 1, IA: 1}, 3: {A: 1}, 4: {A: 1}, 5: {T: 1}, 6: {C: 1}}))


def test_strand_one_insertion_at_j0_is_counted_after_the_right_shift():
    V, Hp = b"AAAACG", b"AAAT"                               # 1I 3= from (0, 0); H = revcomp(H') = ATTT
    H = M.revcomp(Hp)
    assert H == b"ATTT"
    ops = M.parse_cigar("1I3=")
    sL, sR = N.shifts(ops, 0, 0, V, Hp)
    assert sL.tolist() == [0, 0] and sR.tolist() == [3, 0]
    pv, ph, pd = _tables(P.votes, ops, H, V, 1)
    assert pd == 1 and ph[:, IA:].sum() == 0                  # plain: junction 0 of H' = junction lenH of H: dropped
    tv, th, dropped = _tables(N.votes, ops, H, V, 1)
    assert dropped == 0
    assert np.array_equal(th, _table(4, {1: {T: 1, IT: 1}, 2: {T: 1}, 3: {T: 1}}))     # the run now sits before j = 3 of H' = junction 1 of H
    assert np.array_equal(tv, pv) and np.array_equal(tv, _table(6, {0: {DEL: 1}, 1: {A: 1}, 2: {A: 1}, 3: {A: 1}}))


def test_cases_of_the_gpu_test_have_the_shifts_they_are_meant_to_have():
    for c in NC.all_cases():
        nh = sum(int(w) >> 4 for w in c["words"] if (int(w) & 15) != INS)
        nv = sum(int(w) >> 4 for w in c["words"] if (int(w) & 15) != DL)
        M.replay(c["words"], c["Hp"], c["V"], c["tbegH"], c["tbegH"] + nh, c["tbegV"], c["tbegV"] + nv)     # a true alignment
        NC.check_expect(c)
        assert max(len(c["V"]), len(c["Hp"])) <= 320


# ---- properties on random alignments --------------------------------------------------------------------------------------------------
def _random_alignment(rng, nruns, alphabet=b"AC", flank_x=False):
    """(V, H', words): random runs (adjacent ops differ) over a small alphabet, H' derived so that '=' are real matches"""
    ops, prev = [], -1
    for _ in range(nruns):
        choices = [o for o in (EQ, EQ, EQ, X, INS, DL) if o != prev and not (prev >= INS and o >= INS)]
        prev = choices[rng.integers(len(choices))]
        ops.append(prev)
    if flank_x:                                              # every gap between two 'X' runs
        out = []
        for o in ops:
            out += [X, o, X] if o >= INS else [o]
        ops = [o for k, o in enumerate(out) if k == 0 or o != out[k - 1]]
    words = [(int(rng.integers(1, 6 if o == EQ else 3)) << 4) | o for o in ops]
    nV = sum(w >> 4 for w in words if (w & 15) != DL)
    nD = sum(w >> 4 for w in words if (w & 15) == DL)
    t0v, t0h = int(rng.integers(0, 3)), int(rng.integers(0, 3))
    V = NC._rand(rng, t0v + nV + int(rng.integers(0, 3)), alphabet)
    Hp = N.derive_h(V, words, t0v, t0h, rng, dseq=NC._rand(rng, nD, alphabet)) + NC._rand(rng, int(rng.integers(0, 3)), alphabet)
    return V, Hp, np.asarray(words, np.uint32), t0v, t0h


def _flip(words):
    """the runs as the other read sees them: I and D swapped"""
    w = np.asarray(words, np.uint32)
    op = w & 15
    return (w & ~np.uint32(15)) | np.where(op == INS, DL, np.where(op == DL, INS, op)).astype(np.uint32)


def test_property_b_presentation_independence():
    rng = np.random.default_rng(11)
    shifted = 0
    for _ in range(120):
        V, Hp, w, t0v, t0h = _random_alignment(rng, int(rng.integers(1, 30)))
        nv = sum(int(x) >> 4 for x in w if (int(x) & 15) != DL)
        nh = sum(int(x) >> 4 for x in w if (int(x) & 15) != INS)
        # R = V.  (1) as V of a strand-0 pair; (2) as H of a strand-0 pair; (3) as H of a strand-1 pair whose V is revcomp(H')
        as_v, _, _ = _tables(N.votes, w, Hp, V, 0, tbegH=t0h, tbegV=t0v)
        _, as_h0, _ = _tables(N.votes, _flip(w), V, Hp, 0, tbegH=t0v, tbegV=t0h)
        _, as_h1, _ = _tables(N.votes, _flip(w)[::-1], V, M.revcomp(Hp), 1, tbegH=len(V) - t0v - nv, tbegV=len(Hp) - t0h - nh)
        assert np.array_equal(as_v, as_h0) and np.array_equal(as_v, as_h1)
        plain, _, _ = _tables(P.votes, w, Hp, V, 0, tbegH=t0h, tbegV=t0v)
        shifted += int(not np.array_equal(plain, as_v))
    assert shifted > 30                                      # (not vacuous: the normalisation moved something in many of them)


def test_property_a_canonical_position():
    """a gap between two '=' runs that 'X' runs fence off: wherever it sits inside them, the votes are the same"""
    rng = np.random.default_rng(12)
    moved = 0
    for _ in range(150):
        op = (INS, DL)[int(rng.integers(2))]
        L, d, d2 = int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.integers(1, 7))
        head, tail = [(1 << 4) | EQ, (1 << 4) | X], [(1 << 4) | X, (2 << 4) | EQ]
        w = head + [(d << 4) | EQ, (L << 4) | op, (d2 << 4) | EQ] + tail
        V = NC._rand(rng, sum(x >> 4 for x in w if (x & 15) != DL) + 1, b"AC")
        Hp = N.derive_h(V, w, 0, 0, rng, dseq=NC._rand(rng, L, b"AC")) + b"G"
        sL, sR = N.shifts(w, 0, 0, V, Hp)
        ref = [_tables(N.votes, w, M.revcomp(Hp) if s else Hp, V, s) for s in (0, 1)]
        for s in range(-int(sL[3]), int(sR[3]) + 1):          # every other place the same gap can stand
            if s == 0:
                continue
            w2 = [x for x in head + [((d + s) << 4) | EQ, (L << 4) | op, ((d2 - s) << 4) | EQ] + tail if x >> 4]
            M.replay(np.asarray(w2, np.uint32), Hp, V, 0, len(Hp) - 1, 0, len(V) - 1)                       # still a true alignment of the same reads
            for strand in (0, 1):
                got = _tables(N.votes, w2, M.revcomp(Hp) if strand else Hp, V, strand)
                assert np.array_equal(got[0], ref[strand][0]) and np.array_equal(got[1], ref[strand][1])
            moved += 1
    assert moved > 50


def test_properties_c_and_d_idempotence_and_conservation():
    rng = np.random.default_rng(13)
    for _ in range(150):
        V, Hp, w, t0v, t0h = _random_alignment(rng, int(rng.integers(1, 40)))
        sL, sR = N.shifts(w, t0v, t0h, V, Hp)
        # (c) every gap run of the normalised runs is as far as it goes: its shift inside what is left of its '=' neighbour is 0
        wl, wr = N.normalized_words(w, sL), N.normalized_words(w, sR, right=True)
        assert not N.shifts(wl, t0v, t0h, V, Hp)[0].any() and not N.shifts(wr, t0v, t0h, V, Hp)[1].any()
        for strand in (0, 1):
            H = M.revcomp(Hp) if strand else Hp
            nv, nh, nd = _tables(N.votes, w, H, V, strand, tbegH=t0h, tbegV=t0v)
            pv, ph, pd = _tables(P.votes, w, H, V, strand, tbegH=t0h, tbegV=t0v)
            # (d) base + del votes are conserved per read; ins votes: one per gap run but for the junction-len drops
            assert nv[:, :IA].sum() == pv[:, :IA].sum() and nh[:, :IA].sum() == ph[:, :IA].sum()
            gaps = int(((w & 15) >= INS).sum())
            assert nv[:, IA:].sum() + nh[:, IA:].sum() + nd == gaps == pv[:, IA:].sum() + ph[:, IA:].sum() + pd


def test_without_a_slidable_gap_the_votes_are_the_plain_ones():
    rng = np.random.default_rng(14)
    for n in range(60):
        if n % 2:                                            # every gap fenced by 'X' runs, over two letters
            V, Hp, w, t0v, t0h = _random_alignment(rng, int(rng.integers(1, 25)), flank_x=True)
        else:                                                # V cycles ACGT, 'I' runs of 1..3 bases between '=' runs: no period fits
            k = int(rng.integers(1, 12))
            w = []
            for _ in range(k):
                w += [(int(rng.integers(1, 6)) << 4) | EQ, (int(rng.integers(1, 4)) << 4) | INS]
            w = np.asarray(w + [(3 << 4) | EQ], np.uint32)
            t0v, t0h = 1, 2
            V = (b"ACGT" * 40)[:t0v + sum(int(x) >> 4 for x in w) + 2]
            Hp = N.derive_h(V, w, t0v, t0h, rng) + b"T"
        sL, sR = N.shifts(w, t0v, t0h, V, Hp)
        assert not sL.any() and not sR.any()
        for strand in (0, 1):
            H = M.revcomp(Hp) if strand else Hp
            a, b = _tables(N.votes, w, H, V, strand, tbegH=t0h, tbegV=t0v), _tables(P.votes, w, H, V, strand, tbegH=t0h, tbegV=t0v)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- what it buys: DESIGN.md section 21's simulation, scaled down ---------------------------------------------------------------------
def _noisy(t, err, rng):
    out = []
    for c in t:
        r = rng.random()
        if r < err * 0.6:
            out.append(rng.choice(b"ACGT")); out.append(c)
        elif r < err * 0.9:
            continue
        elif r < err:
            out.append(rng.choice([x for x in b"ACGT" if x != c]))
        else:
            out.append(c)
    return bytes(out)


def _simulate(seed, tlen, nreads, err=0.15, k=17, min_depth=3):
    """one template, nreads full-length noisy copies on random strands, every pair traced by the banded mirror from a random shared
    k-mer; summed edit distance of the reads to the template: raw, after the plain consensus, after the normalised one"""
    rng = random.Random(seed)
    tmpl = bytes(rng.choice(b"ACGT") for _ in range(tlen))
    reads, strands = [], []
    for _ in range(nreads):
        s, st = _noisy(tmpl, err, rng), rng.random() < 0.5
        reads.append(M.revcomp(s) if st else s); strands.append(st)
    truth = [M.revcomp(tmpl) if st else tmpl for st in strands]
    off = np.concatenate([[0], np.cumsum([len(s) for s in reads])])
    tabs = {m: np.zeros((int(off[-1]), 9), np.int64) for m in ("plain", "norm")}
    for c in range(nreads):
        idx = {}
        for p in range(len(reads[c]) - k + 1):
            idx.setdefault(reads[c][p:p + k], p)
        for r in range(c + 1, nreads):
            strand = int(strands[c] != strands[r])
            V, Hp = reads[c], M.oriented(reads[r], strand)
            hits = [(idx[Hp[q:q + k]], q) for q in range(len(Hp) - k + 1) if Hp[q:q + k] in idx]
            hits = [(a, b) for a, b in hits if abs(a - b) < 200]
            if not hits:
                continue
            sV, sHp = rng.choice(hits)
            aln = dict(strand=strand, begH=0, begV=0, endH=len(Hp), endV=len(V))
            rec, words, _ = M.trace_expect_banded(reads[r], V, len(Hp) - sHp - k if strand else sHp, sV, k, aln, 256)
            tr = dict(op_off=0, nops=len(words), tbegV=rec["tbegV"], tbegH=rec["tbegH"])
            for m, fn in (("plain", P.votes), ("norm", N.votes)):
                res = fn(words, tr, reads[r], V, strand)
                np.add.at(tabs[m], (off[c] + res[0][0], res[0][1]), 1)
                np.add.at(tabs[m], (off[r] + res[1][0], res[1][1]), 1)
    out = dict(raw=sum(P.edit_distance(reads[r], truth[r]) for r in range(nreads)))
    for m in ("plain", "norm"):
        out[m] = sum(P.edit_distance(P.consensus(reads[r], tabs[m][off[r]:off[r + 1]], min_depth)[0], truth[r]) for r in range(nreads))
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_simulation_normalised_consensus_beats_the_plain_one(seed):
    res = _simulate(seed, tlen=400, nreads=12)
    print("seed %d: raw %d, plain consensus %d, normalised %d (ratio %.2f)" % (seed, res["raw"], res["plain"], res["norm"], res["norm"] / max(1, res["plain"])))
    assert res["norm"] < res["plain"] < res["raw"]


# ---- ABI and command line -------------------------------------------------------------------------------------------------------------
def test_abi_additions(tmp_path):
    lib = _lib.load()
    assert lib.bella_hip_abi_version() == 6
    for name in ("bella_hip_get_vote_stats", "bella_hip_pileup_vote"):
        assert hasattr(lib, name), name
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {',
           'printf("bella_vote_pair size %zu\\n", sizeof(bella_vote_pair));', 'printf("bella_vote_stats size %zu\\n", sizeof(bella_vote_stats));',
           'printf("bella_trace_stats size %zu\\n", sizeof(bella_trace_stats));', 'printf("flag normalize %u\\n", BELLA_TRACE_NORMALIZE);']
    for f in _lib.VOTE_PAIR_DT.names:
        src.append('printf("bella_vote_pair %s %%zu\\n", offsetof(bella_vote_pair, %s));' % (f, f))
    for f, _ in _lib.VoteStats._fields_:
        src.append('printf("bella_vote_stats %s %%zu\\n", offsetof(bella_vote_stats, %s));' % (f, f))
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    assert got[("bella_vote_pair", "size")] == _lib.VOTE_PAIR_DT.itemsize == 32
    assert got[("bella_vote_stats", "size")] == ctypes.sizeof(_lib.VoteStats) == 64
    assert got[("bella_trace_stats", "size")] == ctypes.sizeof(_lib.TraceStats) == 120
    assert got[("flag", "normalize")] == _lib.TRACE_NORMALIZE == 8
    for f in _lib.VOTE_PAIR_DT.names:
        assert got[("bella_vote_pair", f)] == _lib.VOTE_PAIR_DT.fields[f][1], f
    for f, _ in _lib.VoteStats._fields_:
        assert got[("bella_vote_stats", f)] == getattr(_lib.VoteStats, f).offset, f
    assert [f for f, _ in _lib.VoteStats._fields_] == ["pairs", "runs", "gap_runs", "shifted_runs", "shifted_columns", "votes", "vote_ms", "normalized", "pad"]


def test_cli_normalize_gaps_needs_correct_or_polish(tmp_path):
    from bella_amd import build as b
    exe = b.build_cli()
    run = lambda args: subprocess.run([exe, "-f", "in.txt", "-o", "x"] + args, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    p = run(["--normalize-gaps"])
    assert p.returncode == 1 and b"bella-hip:" in p.stderr and b"--normalize-gaps needs --correct or --polish" in p.stderr, p.stderr
    p = run(["--normalize-gaps", "--gfa", "g.gfa"])
    assert p.returncode == 1 and b"--correct" in p.stderr and b"--polish" in p.stderr
    p = run(["--normalize-gaps=1", "--correct", "c.fasta"])
    assert p.returncode == 1 and b"takes no value" in p.stderr
    open(tmp_path / "in.txt", "w").write("/nonexistent/a.fastq")           # no trailing newline: the rules passed, the list names no file
    p = run(["--normalize-gaps", "--correct", "c.fasta"])
    assert p.returncode == 1 and b"no FASTQ file" in p.stderr
    assert b"--normalize-gaps" in run(["--help"]).stdout
