"""TEST TOOLING: a plain numpy restatement of k-mer counting (bella_amd/csrc/kcount.hpp, count_kmers_impl) and a description of what
the device will do with an input.  Nothing under bella_amd/ imports this module.

Part one restates the OPERATION, independent of how the device computes it: the canonical word of every position, the three
selectors (all positions; syncmers with the Murmur first word; the reference's minimizer deque with its size_t range test), the count
per word in 16 bits (wrapping for all positions, saturating for the two selected modes), the reliable set, the dictionary in
ascending order and the tuples in read and position order.  tests/test_kcount_cases_cpu.py holds it against the C oracle.

Part two restates the host's RULES and the run kernels' geometry: plan() (sort-with-positions path or look-up path, position
bits, left-out word bits), passes() (bin ranges under a budget), layout() (the array a pass sorts, its groups with their place in
their tile, their counts per low-bit value, their reliability mask and where they end relative to the tile's look-ahead; per tile
the heads, reliable runs, reliable words and records) and home() (the look-up table's home slot).  The builders of
bella_testkit/kcount_cases.py read their geometry here and raise when an input does not have it; the GPU tests compare plan(),
passes() and the tile counts with what the host reports (Engine.count_stats())."""
from __future__ import annotations

import dataclasses

import numpy as np

U64 = np.uint64
BINS = 256
RUN_TILE, RUN_HALO, RUN_BLOCK = 2048, 32, 256
SMER = 5
HASH_EMPTY = (1 << 64) - 1
DEBUG_LOOKUP = 16384                      # debug bit 14: the look-up path
EMIT_CHUNK = 1024                         # positions a workgroup of k_emit_codes reserves per round


# ---- part one: the operation ------------------------------------------------------------------------------------------------------

def _u(x):
    return np.asarray(x, dtype=U64)


def position_words(rs, k):
    """(forward word, canonical word, read, position) of every k-mer position, read by read, positions ascending"""
    codes = rs.codes.astype(U64)
    offs = np.asarray(rs.offsets, np.int64)
    n = len(codes)
    if n < k:
        z = np.zeros(0, U64)
        return z, z, np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    m = n - k + 1
    fw = np.zeros(m, U64)
    rc = np.zeros(m, U64)
    for j in range(k):
        c = codes[j:j + m]
        fw = (fw << U64(2)) | c
        rc |= (U64(3) - c) << U64(2 * j)
    lens = np.diff(offs)
    nk = np.maximum(lens - k + 1, 0)
    read = np.repeat(np.arange(len(lens), dtype=np.int64), nk)
    koff = np.concatenate([[0], np.cumsum(nk)])
    pos = np.arange(int(koff[-1]), dtype=np.int64) - koff[read]
    start = offs[read] + pos
    fw, rc = fw[start], rc[start]
    return fw, np.minimum(fw, rc), read.astype(np.uint32), pos.astype(np.uint32)


def word_of(s: bytes, k=None):
    """forward word of a string (first base most significant, A C G T = 0 1 2 3)"""
    w = 0
    for ch in (s if k is None else s[:k]):
        w = (w << 2) | b"ACGT".index(ch)
    return w


def string_of(word: int, k: int) -> bytes:
    return bytes(b"ACGT"[(int(word) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def revcomp_word(word: int, k: int) -> int:
    r = 0
    w = int(word)
    for _ in range(k):
        r = (r << 2) | (3 - (w & 3))
        w >>= 2
    return r


def canonical(word: int, k: int) -> int:
    return min(int(word), revcomp_word(word, k))


def _rotl(x, r):
    return (x << U64(r)) | (x >> U64(64 - r))


def _fmix(h):
    h = h ^ (h >> U64(33))
    h = h * U64(0xff51afd7ed558ccd)
    h = h ^ (h >> U64(33))
    h = h * U64(0xc4ceb9fe1a85ec53)
    return h ^ (h >> U64(33))


def kmer_hash(left_aligned):
    """first word of MurmurHash3_x64_128, seed 313, over the 8 bytes of the left-aligned word (arrays of u64; products wrap)"""
    with np.errstate(over="ignore"):
        k1 = np.atleast_1d(_u(left_aligned)).copy()
        h1 = np.full(k1.shape, 313, U64)
        h2 = np.full(k1.shape, 313, U64)
        k1 = k1 * U64(0x87c37b91114253d5)
        k1 = _rotl(k1, 31)
        k1 = k1 * U64(0x4cf5ad432745937f)
        h1 = h1 ^ k1
        h1 = h1 ^ U64(8)
        h2 = h2 ^ U64(8)
        h1 = h1 + h2
        h2 = h2 + h1
        h1, h2 = _fmix(h1), _fmix(h2)
        return h1 + h2


def mix64(x):
    """splitmix64 finaliser (the look-up table's hash)"""
    with np.errstate(over="ignore"):
        x = np.atleast_1d(_u(x)).copy()
        x = x ^ (x >> U64(30))
        x = x * U64(0xbf58476d1ce4e5b9)
        x = x ^ (x >> U64(27))
        x = x * U64(0x94d049bb133111eb)
        return x ^ (x >> U64(31))


def home(words, slots: int):
    return (mix64(words) & U64(slots - 1)).astype(np.int64)


_SMER_TAB = None


def _smer_tab():
    global _SMER_TAB
    if _SMER_TAB is None:
        _SMER_TAB = kmer_hash(np.arange(1 << (2 * SMER), dtype=U64) << U64(64 - 2 * SMER))
    return _SMER_TAB


def is_syncmer(fw, k: int):
    """kept unless an interior s-mer hashes below both end s-mers (on the forward word)"""
    fw = np.atleast_1d(_u(fw))
    tab, last, m = _smer_tab(), k - SMER, U64((1 << (2 * SMER)) - 1)
    st, en = tab[((fw >> U64(2 * last)) & m).astype(np.int64)], tab[(fw & m).astype(np.int64)]
    ok = np.ones(fw.shape, bool)
    for i in range(1, last):
        h = tab[((fw >> U64(2 * (last - i))) & m).astype(np.int64)]
        ok &= ~((h < st) & (h < en))
    return ok


def minimizer_deque(orders, window: int):
    """the reference's getMinimizers on one read's orders (a list of ints): (sampled positions, largest deque length reached).
    The deque is a plain list here, not a ring: what the ring of window + 2 slots must hold is the second return value."""
    dq = []                                            # (position, order)
    out, last, longest = [], -1, 0
    W = int(window)
    for i, o in enumerate(orders):
        while dq and dq[-1][1] > o:
            dq.pop()
        dq.append((i, o))
        longest = max(longest, len(dq))
        bound = (i - W) % (1 << 64)                    # size_t: huge for i < window
        while dq and dq[0][0] <= bound:
            while len(dq) > 1 and dq[0][1] == dq[1][1]:   # furtherPop
                dq.pop(0)
            dq.pop(0)
        if dq and dq[0][0] != last:
            last = dq[0][0]
            out.append(last)
    return out, longest


def select(rs, k, mode, window=0):
    """(fw, canon, read, pos, counted mask, largest deque length per read or None)"""
    fw, canon, read, pos = position_words(rs, k)
    if mode == 0:
        return fw, canon, read, pos, np.ones(len(fw), bool), None
    if mode == 1:
        return fw, canon, read, pos, (is_syncmer(fw, k) if len(fw) else np.zeros(0, bool)), None
    sel = np.zeros(len(fw), bool)
    ords = kmer_hash(canon << U64(64 - 2 * k)) if len(fw) else np.zeros(0, U64)
    nk = np.bincount(read, minlength=rs.nreads)
    koff = np.concatenate([[0], np.cumsum(nk)])
    longest = np.zeros(rs.nreads, np.int64)
    memo = {}
    for r in range(rs.nreads):
        a, b = int(koff[r]), int(koff[r + 1])
        if a == b:
            continue
        key = canon[a:b].tobytes()                     # equal words, equal orders (sets with many copies of a read)
        if key not in memo:
            memo[key] = minimizer_deque([int(x) for x in ords[a:b]], window)
        picks, longest[r] = memo[key]
        sel[a + np.asarray(picks, np.int64)] = True
    return fw, canon, read, pos, sel, longest


def count16(run, saturate):
    run = np.asarray(run, np.int64)
    return np.minimum(run, 65535) if saturate else run & 0xFFFF


@dataclasses.dataclass
class Counted:
    codes: np.ndarray          # the dictionary, ascending
    counts: np.ndarray
    t_kmer: np.ndarray
    t_read: np.ndarray
    t_pos: np.ndarray
    ndistinct: int
    counted_words: np.ndarray  # the word every counted position contributes, in position order
    counted_index: np.ndarray  # ... and its global position index
    npositions: int
    longest_deque: object


def count(rs, k, lower, upper, mode=0, window=0) -> Counted:
    fw, canon, read, pos, sel, longest = select(rs, k, mode, window)
    cw = (fw if mode == 1 else canon)[sel]
    uniq, runs = np.unique(cw, return_counts=True)
    c16 = count16(runs, mode != 0)
    rel = (c16 >= lower) & (c16 <= upper)
    codes, counts = uniq[rel], c16[rel].astype(np.uint16)
    cand = np.ones(len(fw), bool) if mode != 2 else sel   # syncmer mode: EVERY position whose canonical word is a key
    at = np.searchsorted(codes, canon)
    hit = cand & (at < len(codes))
    hit[hit] = codes[at[hit]] == canon[hit]
    return Counted(codes, counts, at[hit].astype(np.uint32), read[hit], pos[hit].astype(np.uint16), len(uniq), cw, np.flatnonzero(sel),
                   len(fw), longest)


# ---- part two: the host's rules and the run kernels' geometry ---------------------------------------------------------------------

def code_bin(words, k):
    words = _u(words)
    return (words >> U64(2 * k - 8) if k >= 4 else words).astype(np.int64)


def plan(ntot, k, mode, debug=0):
    """(fast, pb, gb): the sort-with-positions path, the position bits in its keys, the word bits its sort leaves out"""
    posbits = 1
    while posbits < 63 and (1 << posbits) < ntot:
        posbits += 1
    fast = mode != 1 and 2 * k + posbits <= 64 and posbits <= 32 and not (debug & DEBUG_LOOKUP)
    pb = posbits if fast else 0
    gb = 2 if fast and 2 * k >= 10 and (2 * k + 7) // 8 > (2 * k - 2 + 7) // 8 else 0
    return fast, pb, gb


def passes(hist, budget, mode=None, ntot=None):
    """[(first bin, end bin, words)]: runs of consecutive bins of at most `budget` words (a bin above the budget is a pass of its
    own).  mode 0 with all positions within the budget is one pass over every bin, sized without a histogram."""
    budget = min(int(budget) if budget else 1 << 30, 0x7FFF0000)
    if mode == 0 and ntot is not None and ntot <= budget:
        return [(0, BINS, int(ntot))]
    out, b = [], 0
    while b < BINS:
        n, e = int(hist[b]), b + 1
        while e < BINS and n + int(hist[e]) <= budget:
            n += int(hist[e])
            e += 1
        out.append((b, e, n))
        b = e
    return out


def table_slots(nk):
    slots = 1024
    while slots < 2 * nk:
        slots <<= 1
    return slots


@dataclasses.dataclass
class Layout:
    sorted_words: np.ndarray   # stable by word >> gb
    start: np.ndarray          # per group: index of its first word
    tile: np.ndarray
    e: np.ndarray              # place of the head in its tile
    length: np.ndarray
    cnt: np.ndarray            # [ngroups, 4]
    mask: np.ndarray           # reliable runs of the group, bit v
    end: np.ndarray            # e + length - have of the head's tile: < 0 before, 0 at, > 0 past the look-ahead
    bisects: np.ndarray        # the bisection branch runs (the group reaches `have` and the pass goes on behind it)
    have: np.ndarray           # per tile
    tile_heads: np.ndarray     # runs that start in the tile
    tile_rel: np.ndarray       # reliable runs that start in it
    tile_words: np.ndarray     # their words
    tile_rec: np.ndarray       # groups with a reliable run (records of k_run_assign)

    @property
    def ntiles(self):
        return len(self.have)


def layout(words, pb, gb, lower, upper, saturate) -> Layout:
    """one pass of the sort-with-positions path: `words` in emission order (pb only fixes that the path is taken)"""
    w = _u(words)
    n = len(w)
    order = np.argsort(w >> U64(gb), kind="stable")
    s = w[order]
    g = s >> U64(gb)
    head = np.ones(n, bool)
    head[1:] = g[1:] != g[:-1]
    start = np.flatnonzero(head)
    length = np.diff(np.concatenate([start, [n]]))
    gi = np.cumsum(head) - 1
    v = (s & U64((1 << gb) - 1)).astype(np.int64)
    cnt = np.bincount(gi * 4 + v, minlength=4 * len(start)).reshape(len(start), 4)
    c16 = count16(cnt, saturate)
    relv = (cnt > 0) & (c16 >= lower) & (c16 <= upper)
    mask = (relv * (1 << np.arange(4))).sum(1)
    ntile = -(-n // RUN_TILE)
    x0 = np.arange(ntile, dtype=np.int64) * RUN_TILE
    have = np.minimum(n - x0, RUN_TILE + RUN_HALO)
    tile, e = start // RUN_TILE, start % RUN_TILE
    end = e + length - have[tile]
    bisects = (end >= 0) & (x0[tile] + have[tile] < n)
    per = lambda x: np.bincount(tile, weights=x, minlength=ntile).astype(np.int64)
    return Layout(s, start, tile, e, length, cnt, mask, end, bisects, have, per((cnt > 0).sum(1)), per(relv.sum(1)), per((cnt * relv).sum(1)),
                  per(mask != 0))


def describe(rs, k, lower, upper, mode=0, window=0, debug=0, budget=0):
    """what the device will do with this input: dict(fast, pb, gb, passes, layouts (one per pass with words, None otherwise), slots)"""
    c = count(rs, k, lower, upper, mode, window)
    fast, pb, gb = plan(c.npositions, k, mode, debug)
    hist = np.bincount(code_bin(c.counted_words, k), minlength=BINS)
    ps = passes(hist, budget, mode, c.npositions)
    lays = []
    bins = code_bin(c.counted_words, k)
    for b0, b1, n in ps:
        inpass = (bins >= b0) & (bins < b1)
        assert int(inpass.sum()) == n
        lays.append(layout(c.counted_words[inpass], pb, gb, lower, upper, mode != 0) if fast and n else None)
    return dict(fast=fast, pb=pb, gb=gb, passes=ps, layouts=lays, slots=0 if fast else table_slots(len(c.codes)), counted=c,
                tiles=[(l.ntiles if l is not None else 0) for l in lays])
