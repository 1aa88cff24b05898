"""The synthetic layouts the realignment tests share.  Test tooling: nothing here is used by the product.

line_case(): a line of 6,800 bases.  Five backbone reads of 2,000 bases every 1,200 (ids 1, 3, 5, 7, 9; strands 0, 1, 0, 1, 0: the
unitig runs in the line's direction, so a read's orientation is its strand) and, around them,
    0   [0, 600), strand 1: starts at the unitig's first base; its id is below its backbone read's, so its anchor is H' with strand 1
    2   [1250, 1950): lies in reads 1 and 3 whole -- two candidate anchors of span 700, the tie goes to record (1, 2), whose anchor is V
    4   [6300, 6800): ends at the unitig's last base
    6   [2450, 3150), strand 1: contained in reads 3 and 5
    8   [2500, 2900): its records with backbone reads are taken out; read 6 contains it, nothing places it: UNPLACED
    10  [2600, 3000): likewise, plus a forged record that puts it 1,900 bases into read 9: OUTSIDE
    11  [3700, 5200) with [4300, 4420) deleted from the read; its record's begin point is 10 bases off as well, so at its first base the
        path is 130 diagonals from the centre: with band0 = 256 the band doubles
    12  [3700, 5300) with [4300, 4548) deleted and the same 10 bases: 258 diagonals; with band0 = band_max = 512 it is BAND_CAPPED
    13  800 random bases placed on read 5 by a forged record: LOW_IDENTITY
    14  900 random bases without a record: a one-vertex unitig
The contained reads carry 8 % substitutions (lengths and so the records stay exact).  line_table() deletes every 97th position of the
backbone reads and inserts a C before every 131st, so the polished coordinates are not the raw ones."""
from __future__ import annotations

import numpy as np

from . import graph_mirror as G
from . import unitig_mirror as U

GRAPH = dict(min_overlap=200, fuzz=10)
BACKBONE = (1, 3, 5, 7, 9)


def _mutate(seq: bytes, rate: float, rng) -> bytes:
    a = np.frombuffer(seq, np.uint8).copy()
    hit = np.flatnonzero(rng.random(len(a)) < rate)
    a[hit] = np.frombuffer(b"ACGT", np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", np.uint8), a[hit]) + rng.integers(1, 4, len(hit))) & 3]
    return a.tobytes()


def line_case():
    """-> (seqs, recs): 15 reads and their records"""
    rng = np.random.default_rng(18)
    genome = U.random_genome(6800, 180)
    span = {1: (0, 2000, 0), 3: (1200, 2000, 1), 5: (2400, 2000, 0), 7: (3600, 2000, 1), 9: (4800, 2000, 0),
            0: (0, 600, 1), 2: (1250, 700, 0), 4: (6300, 500, 0), 6: (2450, 700, 1), 8: (2500, 400, 0), 10: (2600, 400, 0)}
    ids = sorted(span)
    starts, lens, strands = ([span[r][k] for r in ids] for k in range(3))
    cut = dict(zip(ids, U.reads_from_genome(genome, starts, lens, strands)))
    recs = G.truth_records(starts, lens, strands, min_overlap=200)
    recs["cid"], recs["rid"] = np.array(ids)[recs["cid"]], np.array(ids)[recs["rid"]]
    lone = lambda r: ((recs["cid"] == r) & np.isin(recs["rid"], BACKBONE)) | ((recs["rid"] == r) & np.isin(recs["cid"], BACKBONE))
    recs = recs[~(lone(8) | lone(10))]
    seqs = [None] * 15
    for r in ids:
        seqs[r] = cut[r] if r in BACKBONE else _mutate(cut[r], 0.08, rng)
    seqs[11] = _mutate(genome[3700:4300] + genome[4420:5200], 0.08, rng)
    seqs[12] = _mutate(genome[3700:4300] + genome[4548:5300], 0.08, rng)
    seqs[13] = U.random_genome(800, 181)
    seqs[14] = U.random_genome(900, 182)
    forged = [(9, 10, 1900, 2000, 0, 390, 0, 0, (0, 0, 0)),           # SHORT for the graph; the only record that joins read 10 to a backbone read
              (7, 11, 390, 1900, 0, 1380, 0, 1, (0, 0, 0)),           # read 7 is the line's reverse complement: [3700, 5200) is [400, 1900) on it
              (7, 12, 290, 1900, 0, 1352, 0, 1, (0, 0, 0)),
              (5, 13, 500, 1300, 0, 800, 0, 0, (0, 0, 0))]
    recs = np.concatenate([recs, np.array(forged, G.OVL_DT)])
    return seqs, recs[np.lexsort((recs["rid"], recs["cid"]))]


def line_table(seqs):
    """(total bases, 9) uint32: on the backbone reads every 97th position is deleted and every 131st has a C inserted before it"""
    lens = np.array([len(s) for s in seqs], np.int64)
    roff = np.concatenate([[0], np.cumsum(lens)])
    t = np.zeros((int(roff[-1]), 9), np.uint32)
    for r in BACKBONE:
        p = np.arange(lens[r])
        own = U._CODE[np.frombuffer(seqs[r], np.uint8)].astype(np.int64)
        g = roff[r] + p
        t[g, own] = 5
        dele = p % 97 == 50
        t[g[dele], 4] = 20
        ins = (p % 131 == 70) & ~dele & ~np.roll(dele, 1)
        t[g[ins], 6] = 10
    return t


def circle_case():
    """12 reads of 1,500 bases every 500 around a circle of 6,000: one circular unitig whose last vertices run across the origin"""
    _, seqs, _, recs = U.circle_input(nreads=12, read_len=1500, step=500, seed=19, fan=2)
    return seqs, recs
