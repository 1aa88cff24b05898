"""Inputs of the affine pair alignment's tests (tests/test_affine_cpu.py, tests/test_affine_gpu.py).  Test tooling:
nothing here is used by the product.

The cases are align_cases' dicts (seqs, pairs, mode, rc, centre, overlap, band0, band_max) and the scorings they run under."""
from __future__ import annotations

import numpy as np

from . import align_cases as AC
from .unitig_mirror import random_genome

LINEAR = (1, 1, 0, 1)
SCORINGS = ((2, 4, 4, 2), (1, 1, 1, 1), (1, 3, 5, 1), (5, 4, 10, 1))      # what the full-matrix Gotoh of the CPU tests is held against
MAIN = (2, 4, 4, 2)
GAPPY = (1, 3, 5, 1)                                                       # a mismatch costs 3, a gap of L bases 5 + L: long indels stay whole
EXTREMES = ((255, 255, 255, 255), (1, 0, 0, 1))


def one_gap(length: int, flank: int, seed: int):
    """(whole, cut, at): `whole` is flank + length + flank bases, `cut` the same without the `length` bases from `at` on.  The bases
    around the block are chosen so that the gap cannot slide: whole[at] != whole[at + length] and whole[at - 1] != whole[at + length - 1]."""
    left = random_genome(flank - 1, seed) + b"A"
    block = b"C" + random_genome(length - 2, seed + 1) + b"T" if length >= 2 else b"C"
    right = b"G" + random_genome(flank - 1, seed + 2)
    return left + block + right, left + right, flank


def gap_case(mode: str, band0: int, length: int, kind: str, flank: int = 200):
    """one pair that differs by a single gap: kind "D" -- the query lacks `length` bases of the target (a run of 'D', F along one row),
    kind "I" -- the target lacks them (a run of 'I', E carried down the rows).  -> (case, the runs every mode must return)"""
    whole, cut, at = one_gap(length, flank, 2900 + 7 * length + band0)
    Q, T = (cut, whole) if kind == "D" else (whole, cut)
    centre = (len(T) - len(Q)) // 2
    op = 3 if kind == "D" else 2
    runs = [at << 4 | 0, length << 4 | op, flank << 4 | 0]
    return AC.case([Q, T], [(0, 1)], mode, centre=centre, band0=band0, band_max=max(band0, 4096)), runs


def seam_lengths(band0: int):
    """gaps that cross one lane boundary (C + 1 cells) and many (70) in the register classes; 300 cells, past a tile of 256, in the wide one"""
    return (band0 // 64 + 1, 70) if band0 <= 1024 else (300,)


# a pair on which the gap-open cost changes the alignment: the query lacks "GT" and "TG" around a kept "CA".  Linear gaps take the two
# short gaps (24 matches - 4 = 20); with o = 6 they would cost 2 * (6 + 2) and leave 8, and one gap of four bases with two mismatches
# (22 - 2 - 10 = 10) is better.  tests/test_affine_cpu.py lists both alignments.
OPEN_Q = b"ACGTACGGTTCA" + b"CA" + b"TTGACCATGA"
OPEN_T = b"ACGTACGGTTCA" + b"GT" + b"CA" + b"TG" + b"TTGACCATGA"


def extreme_case(mode: str):
    """two pairs of about 300 bases at 10 %"""
    rng = np.random.default_rng(2950 + AC.MODES.index(mode))
    seqs, pairs, centres = [], [], []
    for k in range(2):
        Q, T, c = AC.related(mode, 300, rng, 2960 + 10 * AC.MODES.index(mode) + k)
        pairs.append((len(seqs), len(seqs) + 1))
        seqs += [Q, T]
        centres.append(c)
    return AC.case(seqs, pairs, mode, centre=centres, band0=256)


def budget_cases(mode: str):
    """(align_cases.batch_case: twelve pairs of about 500 rows -- 64,000 direction bytes each at a band of 256 and 4 bits a cell, one pair
    a batch under BATCH_BUDGET -- and a pair of 2,000 rows, 256,000 bytes; that pair alone with a first band of 512: 2,000 * 256 bytes)"""
    c = AC.batch_case(mode)
    q, t = c["pairs"][5]
    return c, AC.case([c["seqs"][q], c["seqs"][t]], [(0, 1)], mode, centre=[c["centre"][5]], band0=512)
