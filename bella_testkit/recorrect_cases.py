"""The synthetic layout the correction-round tests share.  Test tooling: nothing here is used by the product.

mixed_case(): eleven reads on a line of 4,000 bases (start, length, strand):
    0   (0, 1500, 0)      1   (300, 1500, 1)      2   (900, 1400, 0)      6   (1900, 1800, 1)
    3   (1000, 512, 0)    exactly two anchor steps; read 0's window on it begins at its first base
    4   (1200, 200, 1)    shorter than one anchor step; every window on it is the whole read, first base to last
    5   [2000, 2600) + [2900, 3500): 300 bases are missing, so against read 6 the path leaves the fixed centre by 150 diagonals: with
        band0 = 256 the band doubles
    7   [2000, 2500) + [3100, 3600): 600 bases are missing: 300 diagonals; with band0 = band_max = 512 both jobs are BAND_CAPPED
    8   800 random bases joined to read 6 by a forged record: LOW_IDENTITY
    9   700 random bases without a record: comes out of a round as it went in
    10  (100, 40, 0), and the round-1 table deletes every position of it: its consensus is empty, the job that targets it is NONE
The records are the exact ones of the pairs that share 150 bases, the four forged ones above and a second, shorter record of the pair
(0, 1).  Every read but 9 carries 6 % substitutions.  mixed_table() gives every read but 9 five votes for its own bases, deletes every
97th position and inserts a C before every 131st, so corrected coordinates are not raw ones."""
from __future__ import annotations

import numpy as np

from . import graph_mirror as G
from . import unitig_mirror as U
from .realign_cases import _mutate

NO_RECORD, EMPTY, SHORT, TWO_STEPS, PAIR_TWICE = 9, 10, 4, 3, (0, 1)
RUNS = {"doubling": dict(band0=256, band_max=2048), "capped": dict(band0=512, band_max=512), "wide": dict(band0=2048, band_max=4096)}


def mixed_case():
    """-> (seqs, recs): 11 reads and their records"""
    rng = np.random.default_rng(20)
    genome = U.random_genome(4000, 200)
    span = {0: (0, 1500, 0), 1: (300, 1500, 1), 2: (900, 1400, 0), 3: (1000, 512, 0), 4: (1200, 200, 1), 6: (1900, 1800, 1)}
    ids = sorted(span)
    starts, lens, strands = ([span[r][k] for r in ids] for k in range(3))
    cut = dict(zip(ids, U.reads_from_genome(genome, starts, lens, strands)))
    recs = G.truth_records(starts, lens, strands, min_overlap=150)
    recs["cid"], recs["rid"] = np.array(ids)[recs["cid"]], np.array(ids)[recs["rid"]]
    seqs = [None] * 11
    for r in ids:
        seqs[r] = _mutate(cut[r], 0.06, rng)
    seqs[5] = _mutate(genome[2000:2600] + genome[2900:3500], 0.06, rng)
    seqs[7] = _mutate(genome[2000:2500] + genome[3100:3600], 0.06, rng)
    seqs[8] = U.random_genome(800, 201)
    seqs[9] = U.random_genome(700, 202)
    seqs[10] = _mutate(genome[100:140], 0.06, rng)
    forged = [(5, 6, 0, 1200, 100, 1600, 0, 1, (0, 0, 0)),            # read 6 is the line's reverse complement: H' = rc(6) runs along the line from 1900
              (6, 7, 100, 1700, 0, 1000, 0, 1, (0, 0, 0)),            # [2000, 3600) of the line is [100, 1700) of read 6 as given
              (6, 8, 200, 1000, 0, 800, 0, 0, (0, 0, 0)),
              (0, 10, 100, 140, 0, 40, 0, 0, (0, 0, 0)),
              (0, 1, 500, 1300, 200, 1000, 0, 1, (0, 0, 0))]          # the pair (0, 1) once more, 800 bases inside its exact record
    recs = np.concatenate([recs, np.array(forged, G.OVL_DT)])
    return seqs, recs[np.lexsort((recs["rid"], recs["cid"]))]


def mixed_table(seqs):
    """(total bases, 9) uint32 for round 1"""
    lens = np.array([len(s) for s in seqs], np.int64)
    roff = np.concatenate([[0], np.cumsum(lens)])
    t = np.zeros((int(roff[-1]), 9), np.uint32)
    for r in range(len(seqs)):
        if r == NO_RECORD:
            continue
        p = np.arange(lens[r])
        own = U._CODE[np.frombuffer(seqs[r], np.uint8)].astype(np.int64)
        g = roff[r] + p
        t[g, own] = 5
        dele = (p % 97 == 50) | (r == EMPTY)
        t[g[dele], 4] = 20
        ins = (p % 131 == 70) & ~dele & ~np.roll(dele, 1)
        t[g[ins], 6] = 10
    return t
