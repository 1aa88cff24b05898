"""Explicit traced pairs that pin the places the normalised vote kernel (pileup.hpp: k_pile_vote_norm) can go
wrong: chunk sizes around 64 runs, shifts across a chunk boundary, gaps without a neighbour, long shifts, periodic repeats, dropped
junctions.  Test tooling.  Every case is built from V and the runs; H' is derived (normalize_mirror.derive_h), so '=' columns are real
matches.  A case is a dict: name, V, Hp (H'), words (uint32 runs), tbegV, tbegH, expect = {run index: (side 'L' / 'R', shift)}."""
from __future__ import annotations

import numpy as np

from . import normalize_mirror as N
from .trace_mirror import revcomp

EQ, X, INS, DEL = 0, 1, 2, 3


def _w(op, ln):
    return (ln << 4) | op


def _case(name, V, words, rng, expect=None, tbegV=0, tbegH=0, dseq=b"", tailH=0):
    Hp = N.derive_h(V, words, tbegV, tbegH, rng, dseq=dseq)
    Hp += bytes(b"ACGT"[rng.integers(4)] for _ in range(tailH))
    return dict(name=name, V=V, Hp=Hp, words=np.asarray(words, np.uint32), tbegV=tbegV, tbegH=tbegH, expect=expect or {})


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(alphabet[rng.integers(len(alphabet))] for _ in range(n))


def run_count_case(nruns: int, rng):
    """nruns runs: '=' 2 alternating with I 1 / X 1 / D 1 over a two-letter V, so about every second gap can slide"""
    words, nV = [], 0
    for k in range(nruns):
        op, ln = (EQ, 2) if k % 2 == 0 else ((INS, X, DEL)[(k // 2) % 3], 1)
        words.append(_w(op, ln))
        nV += ln if op != DEL else 0
    return _case("runs%d" % nruns, _rand(rng, nV + 3, b"AC"), words, rng, dseq=_rand(rng, nruns, b"AC"), tailH=2)


def _prefix(n_runs, first_eq: bool):
    """n_runs runs of one column, '=' and 'X' alternating"""
    return [_w(EQ if (k % 2 == 0) == first_eq else X, 1) for k in range(n_runs)]


def boundary_left_case(full: bool, rng):
    """gap at run 64 whose '=' predecessor is run 63: 0 < sL < d (full=False) or sL == d (full=True)"""
    pre = _prefix(63, first_eq=False)                        # run 62 is 'X'
    body, d, s = (b"AAA", 3, 3) if full else (b"CTAAA", 5, 3)
    words = pre + [_w(EQ, d), _w(INS, 1), _w(EQ, 3)]
    V = _rand(rng, 62) + b"G" + body + b"A" + b"GTC" + _rand(rng, 4)
    c = _case("left64_%s" % ("full" if full else "part"), V, words, rng, expect={64: ("L", s)}, tailH=3)
    assert len(words) == 66 and (int(words[63]) & 15) == EQ and (int(words[62]) & 15) == X
    return c


def boundary_right_case(rng):
    """gap at run 63 whose '=' successor is run 64, sR = 2 (read by the H side of a strand-1 pair)"""
    pre = _prefix(63, first_eq=True)                         # run 62 is '='
    words = pre + [_w(INS, 1), _w(EQ, 4), _w(X, 1), _w(EQ, 2)]
    V = _rand(rng, 62) + b"G" + b"A" + b"AACG" + b"T" + b"CA" + _rand(rng, 3)
    return _case("right63", V, words, rng, expect={63: ("R", 2)}, tailH=3)


def ends_case(rng):
    """gap as first run and gap as last run over a homopolymer: no neighbour on that side, no shift there"""
    words = [_w(INS, 1), _w(EQ, 6), _w(DEL, 1)]
    return _case("ends", b"AAAAAAA" + _rand(rng, 2), words, rng, expect={0: ("L", 0), 2: ("R", 0)}, dseq=b"A", tailH=2)


def between_x_case(rng):
    """gap between 'X' runs inside a homopolymer: it would slide if '=' stood there"""
    words = [_w(EQ, 3), _w(X, 1), _w(INS, 1), _w(X, 1), _w(EQ, 3)]
    return _case("between_x", b"AAAAAAAAA" + _rand(rng, 2), words, rng, expect={2: ("L", 0)}, tailH=1)


def homopolymer_case(rng, right: bool = False):
    """1-base gap at the right end of a 300-base homopolymer: shift 299 (its mirror image for the right shift)"""
    if not right:
        words = [_w(EQ, 300), _w(INS, 1), _w(EQ, 2)]
        return _case("homopolymer_left", b"C" + b"A" * 300 + b"GT" + _rand(rng, 2), words, rng, expect={1: ("L", 299)}, tailH=1)
    words = [_w(EQ, 2), _w(INS, 1), _w(EQ, 300)]
    return _case("homopolymer_right", b"GT" + b"A" * 300 + b"C" + _rand(rng, 2), words, rng, expect={1: ("R", 299)}, tailH=1)


def period3_case(L: int, rng, deletion: bool = False):
    """gap of length L (3: the period, slides over four periods; 2: does not) at the end of G (ACT)x4 ... in a period-3 repeat"""
    rep = b"G" + b"ACT" * 4
    gap = (b"ACT" * 2)[:L]
    if not deletion:
        words = [_w(EQ, len(rep)), _w(INS, L), _w(EQ, 3)]
        V = (b"G" + b"ACT" * 8)[:len(rep) + L + 3] + b"GG"
        return _case("period3_I%d" % L, V, words, rng, expect={1: ("L", 12 if L == 3 else 0)}, tailH=1)
    words = [_w(EQ, len(rep)), _w(DEL, L), _w(EQ, 2)]
    return _case("period3_D%d" % L, rep + b"GG" + _rand(rng, 2), words, rng, expect={1: ("L", 12 if L == 3 else 0)}, dseq=gap, tailH=1)


def junction_h_case(rng):
    """'I' run at j = 0 (read by a strand-1 pair: plain, its ins vote falls on junction lenH of H and is dropped; after the right shift
    it is counted)"""
    return _case("ins_at_j0", b"AAAACG", [_w(INS, 1), _w(EQ, 3)], rng, expect={0: ("R", 3)}, tailH=1)


def junction_v_case(rng):
    """'D' run whose V junction is lenV: plain, its ins vote on V is dropped; H' ends in a homopolymer, so the left shift brings it in"""
    return _case("del_at_lenV", b"GCAAA", [_w(EQ, 5), _w(DEL, 1)], rng, expect={1: ("L", 3)}, dseq=b"A", tailH=2)


def all_cases(seed: int = 7):
    rng = np.random.default_rng(seed)
    cs = [run_count_case(n, rng) for n in (1, 63, 64, 65, 127, 128, 129)]
    cs += [boundary_left_case(False, rng), boundary_left_case(True, rng), boundary_right_case(rng), ends_case(rng), between_x_case(rng),
           homopolymer_case(rng), homopolymer_case(rng, right=True), period3_case(3, rng), period3_case(2, rng), period3_case(3, rng, deletion=True),
           period3_case(2, rng, deletion=True), junction_h_case(rng), junction_v_case(rng)]
    return cs


def check_expect(case, strand: int = 0):
    """the case has the run index and shift it is meant to have"""
    sL, sR = N.shifts(case["words"], case["tbegV"], case["tbegH"], case["V"], case["Hp"])
    for k, (side, s) in case["expect"].items():
        assert (int(case["words"][k]) & 15) >= INS, (case["name"], k)
        got = int(sL[k]) if side == "L" else int(sR[k])
        assert got == s, (case["name"], k, side, got, s)
    return sL, sR


def build_batch(cases, strands_roles):
    """Reads, vote pairs (dtype of bella_vote_pair) and the op array of one explicit batch: case n is voted as pair n with
    (strand, v_first) = strands_roles[n % len]: H = H' or its reverse complement, V before H in the read set (cid < rid) or behind."""
    from bella_amd import _lib
    reads, recs, ops = [], [], []
    for n, c in enumerate(cases):
        strand, v_first = strands_roles[n % len(strands_roles)]
        H = revcomp(c["Hp"]) if strand else c["Hp"]
        iv, ih = (len(reads), len(reads) + 1) if v_first else (len(reads) + 1, len(reads))
        reads += [c["V"], H] if v_first else [H, c["V"]]
        r = np.zeros(1, _lib.VOTE_PAIR_DT)[0]
        r["rid"], r["cid"], r["tbegV"], r["tbegH"], r["op_off"], r["nops"], r["strand"] = ih, iv, c["tbegV"], c["tbegH"], sum(len(o) for o in ops), len(c["words"]), strand
        recs.append(r)
        ops.append(c["words"])
    pairs = np.array(recs, _lib.VOTE_PAIR_DT) if recs else np.zeros(0, _lib.VOTE_PAIR_DT)
    return reads, pairs, (np.concatenate(ops).astype(np.uint32) if ops else np.zeros(0, np.uint32))


def mirror_table(reads, pairs, ops, normalize: bool):
    """the table of an explicit batch by the mirrors: (table uint32, stats dict as bella_vote_stats counts)"""
    from . import pileup_mirror as P
    lens = np.array([len(s) for s in reads], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    flat = []
    tot = dict(pairs=0, runs=0, gap_runs=0, shifted_runs=0, shifted_columns=0, votes=0)
    for p in pairs:
        if not int(p["nops"]):
            continue
        rid, cid, strand = int(p["rid"]), int(p["cid"]), int(p["strand"])
        if normalize:
            (pV, cV), (pH, cH), _, st = N.votes(ops, p, reads[rid], reads[cid], strand)
            for k, v in st.items():
                tot[k] += v
        else:
            (pV, cV), (pH, cH), _ = P.votes(ops, p, reads[rid], reads[cid], strand)
            tot["runs"] += int(p["nops"])
        tot["pairs"] += 1
        tot["votes"] += len(pV) + len(pH)
        flat += [(off[cid] + pV) * P.NCOUNTERS + cV, (off[rid] + pH) * P.NCOUNTERS + cH]
    idx = np.concatenate(flat).astype(np.int64) if flat else np.zeros(0, np.int64)
    return np.bincount(idx, minlength=int(off[-1]) * P.NCOUNTERS).reshape(-1, P.NCOUNTERS).astype(np.uint32), tot
