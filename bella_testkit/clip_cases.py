"""Inputs of tests/test_clip_gpu.py: hand-made run lists that put the clip's decisions at the places the kernel
can go wrong -- the 64-run chunk borders, the tie rules, 64-bit sums -- each with the (a, b) it is meant to have, random pairs, and
the synthetic reads with junk ends of the effect test.  tests/test_clip_cpu.py checks the expectations against the mirror."""
import numpy as np

from bella_amd import _lib
from bella_testkit import synth

EQ, X, INS, DEL = 0, 1, 2, 3
RUN_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
BATCH_SIZES = (1, 3, 4, 5, 257)
IDENTITIES = (1, 350, 500, 650, 999)


def w(length, op):
    return (int(length) << 4) | op


def poor(n, last=X):
    """n runs of alternating 'X' 1 and '=' 1 whose last run is `last`: every step loses at t >= 500 (350 - 650 at the default)"""
    ops = [last if (n - 1 - k) % 2 == 0 else (EQ if last == X else X) for k in range(n)]
    return [w(1, o) for o in ops]


def good(n, first=EQ):
    """n runs of alternating '=' 10 and 'X' 1 that begin with `first`: every pair of them gains"""
    return [w(10, EQ) if (k % 2 == 0) == (first == EQ) else w(1, X) for k in range(n)]


def random_runs(rng, n, maxlen=12):
    out, prev = [], -1
    for _ in range(n):
        op = int(rng.choice([o for o in (EQ, EQ, EQ, X, INS, DEL) if o != prev]))
        out.append(w(rng.integers(1, maxlen + 1 if op == EQ else 4), op))
        prev = op
    return out


def hand_cases():
    """[(name, identity, words, expected (a, b) or None for whatever the mirror says)]"""
    rng = np.random.default_rng(24)
    out = [("count%d" % n, 650, random_runs(rng, n), None) for n in RUN_COUNTS]
    out += [
        ("in chunk 0", 650, poor(10) + [w(100, EQ)] + poor(189)[::-1], (10, 11)),
        ("in chunk 2", 650, poor(140) + [w(100, EQ)] + poor(59)[::-1], (140, 141)),
        ("chunk 0 into chunk 2", 650, poor(5) + good(145) + poor(50)[::-1], (5, 150)),
        ("minimum at run 63", 650, poor(63) + [w(50, EQ), w(1, X), w(3, EQ), w(9, X)], (63, 66)),
        ("minimum at run 64", 650, poor(64) + [w(50, EQ), w(1, X), w(3, EQ), w(9, X)], (64, 67)),
        ("best end at run 63", 650, poor(63) + [w(50, EQ)] + poor(40)[::-1], (63, 64)),
        ("best end at run 64", 650, poor(64) + [w(50, EQ)] + poor(40)[::-1], (64, 65)),
        ("minimum in chunk 0, best end in chunk 3", 650, poor(30) + good(171) + [w(9, X), w(1, EQ)], (30, 201)),
        ("two equal segments", 650, [w(1, X), w(10, EQ), w(20, X), w(10, EQ), w(1, X)], (1, 2)),
        ("two equal segments, chunks apart", 650, [w(1, X), w(10, EQ)] + poor(99) + [w(10, EQ), w(1, X)], (1, 2)),
        ("zero sum in front", 500, [w(1, EQ), w(1, X), w(5, EQ)], (2, 3)),
        ("zero sum in front, across a chunk border", 500, poor(64, last=X)[1:] + [w(1, EQ), w(1, X)] + [w(5, EQ)], (65, 66)),
        ("zero sum behind", 500, [w(5, EQ), w(1, X), w(1, EQ)], (0, 1)),
        ("zero sum behind, across a chunk border", 500, [w(5, EQ)] + poor(130, last=EQ), (0, 1)),
        ("alternating at 500", 500, [w(1, EQ) if k % 2 == 0 else w(1, X) for k in range(130)], (0, 1)),
        ("no match at all", 650, [w(3, X), w(2, INS), w(4, DEL)], (0, 0)),
        ("no match at all, three chunks", 650, [w(1 + k % 3, (X, INS, DEL)[k % 3]) for k in range(150)], (0, 0)),
        ("a single run", 650, [w(7, EQ)], (0, 1)),
        ("a single mismatch", 650, [w(7, X)], (0, 0)),
        ("2^24 columns", 650, [w(3, X), w(1 << 24, EQ), w(2, X)], (1, 2)),
        # (the halves do not join: 2^24 x 650 outweighs 2^24 x 350; the later half wins by one column, 350 in 5,872,025,950)
        ("2^24 columns lost against 2^24 mismatches", 650, [w(1 << 24, EQ), w(1 << 24, X), w((1 << 24) + 1, EQ)], (2, 3)),
        ("2^26 columns at 999", 999, [w(1 << 26, EQ), w(1 << 16, INS), w(1 << 26, EQ), w(1 << 17, DEL), w(5, EQ)], (0, 3)),
        ("longest runs of the format", 1, [w((1 << 28) - 1, EQ), w(1 << 20, X), w((1 << 28) - 1, EQ)], (0, 3)),
    ]
    return out


def build_batch(word_lists, seed=7):
    """-> (pairs VOTE_PAIR_DT, ops uint32): one pair per list at a random (tbegV, tbegH), a few spare runs between the pairs' runs"""
    rng = np.random.default_rng(seed)
    pairs = np.zeros(len(word_lists), _lib.VOTE_PAIR_DT)
    ops = []
    for q, words in enumerate(word_lists):
        ops += [w(3, X)] * int(rng.integers(0, 3))
        pairs[q]["op_off"], pairs[q]["nops"] = len(ops), len(words)
        pairs[q]["tbegV"], pairs[q]["tbegH"] = int(rng.integers(0, 1000)), int(rng.integers(0, 1000))
        pairs[q]["rid"], pairs[q]["cid"], pairs[q]["strand"] = q + 1, q, q & 1               # (not read by the clip)
        ops += list(words)
    ops += [w(2, DEL)]
    return pairs, np.asarray(ops, np.uint32)


def random_batch(n=2000, max_runs=300, seed=5):
    rng = np.random.default_rng(seed)
    return build_batch([random_runs(rng, int(rng.integers(0, max_runs + 1)), maxlen=int(rng.integers(2, 16))) for _ in range(n)], seed)


# ---- the effect test: reads of a random genome, 15 % error, junk of random bases on 40 % of the ends ------------------------------------
def junk_reads(nreads=300, read_len=5000, coverage=30.0, err=0.15, frac=0.4, lo=600, hi=1500, seed=31):
    """-> (ReadSet with the junk, head[nreads], tail[nreads], length without junk[nreads]): the true clip of read r is (head[r], head[r] + len[r])"""
    rs = synth.make_reads(nreads, read_len=read_len, coverage=coverage, err=err, seed=seed)
    rng = np.random.default_rng(seed + 1)
    head = np.where(rng.random(nreads) < frac, rng.integers(lo, hi + 1, nreads), 0)
    tail = np.where(rng.random(nreads) < frac, rng.integers(lo, hi + 1, nreads), 0)
    seqs = rs.seqs()
    lens = np.asarray([len(s) for s in seqs], np.int64)
    junk = lambda n: synth.BASES[rng.integers(0, 4, int(n), dtype=np.uint8)].tobytes()
    out = [junk(h) + bytes(s) + junk(t) for s, h, t in zip(seqs, head, tail)]
    return synth.readset_from_seqs(out, list(rs.names)), head, tail, lens
