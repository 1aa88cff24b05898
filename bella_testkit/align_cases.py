"""Inputs of the pair alignment's tests (tests/test_align_cpu.py, tests/test_align_gpu.py): small synthetic
sequences with known edits.  Test tooling: nothing here is used by the product.

A case is a dict(seqs, pairs, mode, rc, centre, overlap, band0, band_max): what Engine.align_sequences takes (align_mirror.records_of
turns it into the records of the C call).  Sequences are 1 .. 2,000 bases."""
from __future__ import annotations

import numpy as np

from .trace_mirror import revcomp
from .unitig_mirror import random_genome

MODES = ("global", "semiglobal", "dovetail")


def case(seqs, pairs, mode, rc=None, centre=None, overlap=None, band0=512, band_max=4096):
    return dict(seqs=list(seqs), pairs=list(pairs), mode=mode, rc=rc, centre=centre, overlap=overlap, band0=band0, band_max=band_max)


def noisy(seq: bytes, rate: float, rng, mix=(0.4, 0.3, 0.3)):
    """seq with substitutions, inserted and deleted bases at `rate` per base (split by `mix`): (copy, [substituted, inserted, deleted])"""
    out, cnt = [], [0, 0, 0]
    p_sub, p_ins, p_del = (rate * x for x in mix)
    for ch in seq:
        x = rng.random()
        if x < p_del:
            cnt[2] += 1
            continue
        if x < p_del + p_sub:
            out.append(b"ACGT"[(b"ACGT".index(ch) + int(rng.integers(1, 4))) & 3])
            cnt[0] += 1
        else:
            out.append(ch)
        if p_del + p_sub <= x < p_del + p_sub + p_ins:
            out.append(b"ACGT"[int(rng.integers(0, 4))])
            cnt[1] += 1
    return bytes(out) or seq[:1], cnt


def related(mode: str, n: int, rng, seed: int, rate=0.10):
    """(Q, T, centre) of about n rows, related as the mode aligns them, with `rate` substitutions and indels.  global: T is a noisy copy
    of Q; semiglobal: Q is a noisy copy of a window of T that starts at `centre`; dovetail: a prefix of Q is a noisy copy of a suffix of
    T, and the centre is m - (the suffix's length)."""
    if mode == "global":
        Q = random_genome(n, seed)
        T, _ = noisy(Q, rate, rng)
        return Q, T, (len(T) - len(Q)) // 2
    if mode == "semiglobal":
        a, z = int(rng.integers(0, 200)), int(rng.integers(0, 200))
        T = random_genome(a + n + z, seed)
        Q, _ = noisy(T[a:a + n], rate, rng)
        return Q, T, a
    ovl = int(rng.integers(n // 3, n + 1))
    t = random_genome(ovl, seed)
    T = random_genome(int(rng.integers(1, 300)), seed + 1) + t
    Q = noisy(t, rate, rng)[0] + random_genome(n - ovl + 1, seed + 2)
    return Q, T, len(T) - ovl


def band_class_case(mode: str, band0: int):
    """one call per mode and first band: 256, 512 and 1,024 run the three register kernels on four pairs of 300 .. 700 bases, 2,048 the
    wide one on one pair of 600 rows"""
    rng = np.random.default_rng(2800 + band0 + MODES.index(mode))
    seqs, pairs, centres = [], [], []
    for k in range(4 if band0 <= 1024 else 1):
        n = int(rng.integers(300, 701)) if band0 <= 1024 else 600
        Q, T, c = related(mode, n, rng, 100 * band0 + 10 * MODES.index(mode) + k)
        if band0 > 1024:
            Q = (Q + random_genome(600, 7))[:600]
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [Q, T]
        centres.append(c)
    return case(seqs, pairs, mode, centre=centres, band0=band0, band_max=max(band0, 4096))


def _block(extra: int, seed: int):
    """(Q, T): T of 700 bases, Q the same with `extra` foreign bases inserted after base 350"""
    T = random_genome(700, seed)
    return T[:350] + random_genome(extra, seed + 1) + T[350:], T


def edge_cases():
    """name -> case.  The statuses and bands some of them are built to produce are asserted in tests/test_align_cpu.py from the mirror."""
    g = lambda n, s: random_genome(n, s)
    out = {}
    for mode in MODES:
        ov = dict(overlap=1) if mode == "dovetail" else {}
        out["one_base_match_" + mode] = case([b"G", b"G"], [(0, 1)], mode, band0=256, **ov)
        out["one_base_mismatch_" + mode] = case([b"G", b"T"], [(0, 1)], mode, band0=256, **ov)
        out["one_against_600_" + mode] = case([b"A", g(600, 11)], [(0, 1)], mode, band0=256, **ov)
        out["600_against_one_" + mode] = case([g(600, 12), b"C"], [(0, 1)], mode, band0=256, **ov)
        same = g(500, 13)
        out["identical_" + mode] = case([same, same], [(0, 1)], mode, band0=256, **(dict(overlap=500) if mode == "dovetail" else {}))
        out["nothing_in_common_" + mode] = case([b"A" * 300, b"C" * 300], [(0, 1)], mode, band0=256, **(dict(overlap=150) if mode == "dovetail" else {}))
    t = g(800, 14)
    # global, m - n = 300 at band0 256: the centre is 150, the start (0, 0) lies outside the first band, which doubles once without a DP
    out["global_start_outside_the_first_band"] = case([t[:250] + t[550:], t], [(0, 1)], "global", band0=256)
    # global, m - n = 600 at band_max 512: neither the start nor the end fits
    out["global_capped_before_any_dp"] = case([t[:100] + t[700:], t], [(0, 1)], "global", band0=256, band_max=512)
    # a block of 120 foreign bases in Q, centre 8: the path leaves the block on diagonal -120, position 0 of a band of 256
    for mode in ("global", "semiglobal"):
        out["block_120_doubles_the_band_" + mode] = case(_block(120, 15), [(0, 1)], mode, centre=8, band0=256)
        out["block_248_is_capped_at_512_" + mode] = case(_block(248, 16), [(0, 1)], mode, centre=8, band0=256, band_max=512)
    out["dovetail_best_cell_in_row_0"] = case([b"C" * 200, g(300, 17).replace(b"C", b"A")], [(0, 1)], "dovetail", overlap=100, band0=256)
    rng = np.random.default_rng(18)
    for mode in MODES:
        Q, T, c = related(mode, 500, rng, 19 + MODES.index(mode))
        out["centre_off_by_100_" + mode] = case([Q, T], [(0, 1)], mode, centre=c + 100, band0=256)
    return out


def rc_case(mode: str):
    """(with the flag, with the query reverse-complemented by hand): six pairs each, the same answers"""
    rng = np.random.default_rng(2900 + MODES.index(mode))
    seqs, flagged, pairs, centres = [], [], [], []
    for k in range(6):
        Q, T, c = related(mode, int(rng.integers(100, 600)), rng, 500 + 10 * MODES.index(mode) + k)
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [Q, T]
        flagged += [revcomp(Q), T]
        centres.append(c)
    return case(flagged, pairs, mode, rc=True, centre=centres, band0=256), case(seqs, pairs, mode, centre=centres, band0=256)


def reuse_case():
    """one target of 1,500 bases used by 50 semi-global pairs, every fifth query reverse-complemented, the pairs in shuffled order"""
    rng = np.random.default_rng(3000)
    T = random_genome(1500, 3001)
    seqs, pairs, centres, rc = [T], [], [], []
    for k in range(50):
        a, n = int(rng.integers(0, 1200)), int(rng.integers(50, 300))
        Q, _ = noisy(T[a:a + n], 0.08, rng)
        rc.append(k % 5 == 0)
        seqs.append(revcomp(Q) if rc[-1] else Q)
        pairs.append((k + 1, 0))
        centres.append(a)
    order = rng.permutation(50)
    return case(seqs, [pairs[i] for i in order], "semiglobal", rc=[rc[i] for i in order], centre=[centres[i] for i in order], band0=256)


def mixed_case(mode: str):
    """lengths from 1 to 2,000 in one call, default centres (overlap for the dovetail): some pairs double their band"""
    rng = np.random.default_rng(3100 + MODES.index(mode))
    seqs, pairs, ovl = [], [], []
    for k, n in enumerate((1, 2, 17, 64, 255, 256, 257, 1000, 1999, 2000, 33, 700)):
        Q, T, c = related(mode, n, rng, 3200 + 20 * MODES.index(mode) + k, rate=0.06)
        ovl.append(min(len(T) - c, 2000))                             # (of a dovetail: the suffix of T that was planted)
        if k in (7, 9):                                               # 260 foreign bases in Q: a band of 256 cannot follow them
            Q = Q[:len(Q) // 4] + random_genome(260, 3300 + k) + Q[len(Q) // 4:]
        Q, T = Q[:2000], T[-2000:]
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [Q, T]
    return case(seqs, pairs, mode, overlap=ovl if mode == "dovetail" else None, band0=256)


BATCH_BUDGET = 100_000      # direction bytes: three pairs of about 500 rows at a band of 256 (32,000 bytes each) fill a batch


def batch_case(mode: str):
    """twelve pairs of about 500 rows and one of 2,000 (128,000 direction bytes at a band of 256): under BATCH_BUDGET four batches or
    more, and the large pair is TOO_LARGE"""
    rng = np.random.default_rng(3300 + MODES.index(mode))
    seqs, pairs, centres = [], [], []
    for k in range(13):
        Q, T, c = related(mode, 2000 if k == 5 else int(rng.integers(450, 500)), rng, 3400 + 20 * MODES.index(mode) + k, rate=0.05 if k != 5 else 0.0)
        if k == 5:
            Q, T = Q[:2000], T[:2000]
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [Q, T]
        centres.append(min(c, len(T)))
    return case(seqs, pairs, mode, centre=centres, band0=256)


def identity_case():
    """20 templates of 2,000 bases and a copy of each with known edits: (queries, templates, [substituted, inserted, deleted] per pair)"""
    rng = np.random.default_rng(3500)
    queries, templates, edits = [], [], []
    for k in range(20):
        T = random_genome(2000, 3600 + k)
        Q, cnt = noisy(T, 0.002 * (k + 1), rng)
        queries.append(Q)
        templates.append(T)
        edits.append(cnt)
    return queries, templates, edits
