"""Which branch of operand assembly an input takes (assemble.hpp, slotorder.hpp; bella_hip.hip: assemble_rows_device, build_layout),
restated in numpy / plain Python.  Test tooling: nothing here is used by the product.

Only what DECIDES a branch is restated -- table sizes and classes, round bounds, probe chains, the LDS window of k_layout_emit, the steps
of run_bounds, chunk and round totals -- so that a case builder can read its geometry back and a test can hold the device's report
(Engine.assemble_stats()) against it.  The answers themselves come from the oracle (tests/_oracle.py).  The one thing simulated in full is
the slot order of a read's table (sequential linear probing, CSC.cpp:316-375), because probe lengths and wraps fall out of it; the CPU
tests compare it with the oracle's rows."""
from __future__ import annotations

import numpy as np

K_PRE = 4                                   # asm_row: k-mer ids held in registers per thread
ASM_GRID = 128                              # bella_hip.hip: kAsmGrid, workgroups of the global class
CLASS_HT = (1024, 2048, 4096, 8192)         # asm_class_of
CLASS_BLK = (256, 512, 1024, 1024, 1024)    # workgroup size per class
EMIT_HALO = 32                              # kEmitHalo
EMIT_BLOCKS = (256, 1024)                   # k_layout_emit: default launch, partitioned launch
LINEAR_STEPS = 16                           # run_bounds
MAX_DEGREE = 16383                          # Bent's product count field holds 14 bits
ROWLIST_BLOCK = 1024                        # kRowListBlock
CHUNK = 64                                  # k_layout_compact_products, k_layout_compact
M32 = 0xFFFFFFFF


def pow2_at_least(minsz: int, n: int) -> int:
    s = minsz
    while s < n:
        s <<= 1
    return s


def asm_class_of(ht: int) -> int:
    return 0 if ht <= 1024 else 1 if ht <= 2048 else 2 if ht <= 4096 else 3 if ht <= 8192 else 4


def asm_dedup_slots(n: int) -> int:
    return ((n * 7 + 4) // 5) | 1


def hash_range(key: int, size: int) -> int:
    return (((key * 2654435761) & M32) * size) >> 32


def slot_home(key: int, ht: int) -> int:
    return ((key * 107) & M32) & (ht - 1)


def round_bound(r: int, ht: int, d: int, tmax: int) -> int:
    keep = ht >> (r + 2) if r + 2 < 32 else 0
    if keep < 32:
        return tmax
    b = tmax * (ht - keep) // (d if d else 1)
    return tmax if b >= tmax else b


def round_bounds(ht: int, d: int, n: int) -> list:
    """the bounds asm_row's round loop runs through (the last one is n)"""
    out, r = [], 0
    while True:
        b = round_bound(r, ht, d, n)
        out.append(b)
        if b >= n:
            return out
        r += 1


class _Table:
    """a table filled by sequential linear probing; the probe is a jump to the next free slot (a union-find over the occupied runs), so
    that a read whose k-mers all share a home costs n steps, not n * n / 2"""

    def __init__(self, size: int):
        self.size, self.item, self.free = size, [None] * size, size
        self.nxt = list(range(size + 1))                               # nxt[s]: a slot >= s that may be free; size: past the end

    def _find(self, s: int) -> int:
        nxt, root = self.nxt, s
        while nxt[root] != root:
            root = nxt[root]
        while nxt[s] != root:
            nxt[s], s = root, nxt[s]
        return root

    def insert(self, home: int, item) -> tuple:
        """-> (slot, steps past the home slot, wrapped the table end)"""
        assert self.free
        s, wrapped = self._find(home), False
        if s == self.size:
            s, wrapped = self._find(0), True
        self.item[s] = item
        self.nxt[s] = s + 1
        self.free -= 1
        return s, (s - home) % self.size, wrapped

    def last_free(self) -> int:
        s = self.size - 1
        while s >= 0 and self.item[s] is not None:
            s -= 1
        return s


class ReadGeometry:
    """one read's tuples (k-mer ids in tuple order) -> what asm_row does with them"""

    def __init__(self, kmers):
        kmers = [int(x) for x in kmers]
        n = self.n = len(kmers)
        assert 0 < n < 65536
        self.ht = pow2_at_least(16, n)
        self.cls = asm_class_of(self.ht)
        self.blk = CLASS_BLK[self.cls]
        self.KS = asm_dedup_slots(self.ht if self.cls < 4 else n)
        first, last = {}, {}
        for t, km in enumerate(kmers):
            first.setdefault(km, t)
            last[km] = t
        self.first, self.last = first, last
        self.d = len(first)
        self.dup = self.d < n
        self.bounds = round_bounds(self.ht, self.d, n)
        self.rounds = len(self.bounds)
        self.beyond_prefetch = n > K_PRE * self.blk
        # the distinct k-mers per round: those whose first occurrence lies in [previous bound, bound)
        firsts = np.sort(np.fromiter(first.values(), np.int64, self.d))
        self.round_items = np.diff(np.searchsorted(firsts, [0] + self.bounds)).tolist()
        # the reference's table: distinct k-mers in the order of their first occurrences, linear probing from key * 107
        table = _Table(self.ht)
        self.slot_chain, self.slot_wraps, self.slot_homes = 0, False, set()
        for km, t in first.items():                                    # (dicts keep insertion order = first-occurrence order)
            home = slot_home(km, self.ht)
            self.slot_homes.add(home)
            _, steps, wrapped = table.insert(home, km)
            self.slot_chain = max(self.slot_chain, steps)
            self.slot_wraps |= wrapped
        self.slot_order = [km for km in table.item if km is not None]
        # free slots at the start of each later round lie only BEFORE the homes of that round's items: build_next_free wraps
        self.next_free_wraps = self._next_free_wraps(kmers)
        # the de-duplication table: which slots end up occupied does not depend on the insertion order, nor does whether a key went
        # round the table end; the chain length is that of insertion in tuple order
        dtab = _Table(self.KS)
        self.dedup_chain, self.dedup_wraps = 0, False
        for km in first:
            _, steps, wrapped = dtab.insert(hash_range(km, self.KS), km)
            self.dedup_chain = max(self.dedup_chain, steps)
            self.dedup_wraps |= wrapped

    def _next_free_wraps(self, kmers) -> bool:
        if self.rounds < 2:
            return False
        table = _Table(self.ht)
        order = sorted(self.first.items(), key=lambda kv: kv[1])
        x, wraps = 0, False
        for rd, bound in enumerate(self.bounds):
            if rd:
                last_free = table.last_free()
                for km, t in order[x:]:
                    if t >= bound:
                        break
                    if last_free >= 0 and slot_home(km, self.ht) > last_free:
                        wraps = True
            while x < len(order) and order[x][1] < bound:
                table.insert(slot_home(order[x][0], self.ht), order[x][0])
                x += 1
        return wraps

    def row(self, kmers, pos):
        """(k-mer ids, positions) of the read's row of B: slot order, the LAST occurrence's position"""
        return (np.asarray(self.slot_order, np.uint32), np.asarray([int(pos[self.last[km]]) for km in self.slot_order], np.uint16))


def rows_geometry(nreads: int, tk, tr) -> dict:
    """{read: ReadGeometry} of every read with tuples (tuples grouped by non-decreasing read id)"""
    tr = np.asarray(tr, np.int64)
    starts = np.searchsorted(tr, np.arange(nreads + 1))
    return {r: ReadGeometry(tk[starts[r]:starts[r + 1]]) for r in range(nreads) if starts[r + 1] > starts[r]}


def class_counts(geo: dict) -> tuple:
    c = [0] * 5
    for g in geo.values():
        c[g.cls] += 1
    return tuple(c)


def global_schedule(geo: dict) -> list:
    """the reads of the global class per workgroup of k_asm_rows_global, in the order it takes them -- for ANY order in which k_asm_classify
    listed them this is a property only of the list position, so the mirror states the workgroups' loads: how many take 1, 2, ... reads"""
    n = sum(1 for g in geo.values() if g.cls == 4)
    grid = min(n, ASM_GRID)
    return [len(range(w, n, grid)) for w in range(grid)]


# ---- canonical k-mers of a sequence --------------------------------------------------------------------------------------------------
_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def kmer_codes(seq: bytes, k: int):
    """(forward, reverse-complement) 2-bit codes, first base most significant, of every k-mer of seq (uint64 arrays, len - k + 1)"""
    c = _CODE[np.frombuffer(seq, np.uint8)].astype(np.uint64)
    m = len(c) - k + 1
    if m <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    fw = np.zeros(m, np.uint64)
    rc = np.zeros(m, np.uint64)
    for i in range(k):
        fw |= c[i:i + m] << np.uint64(2 * (k - 1 - i))
        rc |= (np.uint64(3) - c[i:i + m]) << np.uint64(2 * i)
    return fw, rc


# ---- the layout ----------------------------------------------------------------------------------------------------------------------
def bits_for(n: int) -> int:
    """build_layout: kbits for nkmers, ebits for the owned nonzeros"""
    b = 1
    while b < 32 and (1 << b) < n:
        b += 1
    return b


class LayoutGeometry:
    """the CSR of B (Bc row pointers per read, Br k-mer ids in row order) + which k-mers are palindromes -> per sorted entry, per chunk,
    per round what the layout kernels do.  first / stride: the partition (set_partition) whose B' is built."""

    def __init__(self, Bc, Br, nkmers: int, pal_of_kmer=None, first: int = 0, stride: int = 1):
        Bc = np.asarray(Bc, np.int64)
        Br = np.asarray(Br, np.int64)
        self.nreads, self.nnz, self.nkmers = len(Bc) - 1, len(Br), nkmers
        self.first, self.stride = first, stride
        rows = np.repeat(np.arange(self.nreads), np.diff(Bc))
        order = np.argsort(Br, kind="stable")
        self.skey = Br[order]
        self.sread = rows[order]
        self.sentry = order                                            # the entry of B a sorted place holds
        x = np.arange(self.nnz)
        self.lo = np.searchsorted(self.skey, self.skey, "left")
        self.hi = np.searchsorted(self.skey, self.skey, "right")
        self.degree = self.hi - self.lo
        self.rank = x - self.lo
        pal = np.zeros(max(nkmers, 1), bool)
        if pal_of_kmer is not None:
            pal[:len(pal_of_kmer)] = pal_of_kmer
        self.pal = pal[self.skey] if self.nnz else np.zeros(0, bool)
        self.inline_eligible = (self.rank + 2 == self.degree) & ~self.pal
        self.later = self.degree - 1 - self.rank                       # reads after this one in the k-mer's list
        self.kbits = bits_for(nkmers)
        owned = self.sread % stride == first
        self.nown = int(owned.sum())
        self.ebits = bits_for(self.nown)
        self.place_sorts = self.nown > 0 and self.ebits > 12
        self.over_degree = bool(self.nnz and self.degree.max() > MAX_DEGREE)
        self.blk = EMIT_BLOCKS[1] if stride > 1 else EMIT_BLOCKS[0]
        # per entry of B (row order): later reads of its k-mer
        self.later_of_entry = np.zeros(self.nnz, np.int64)
        self.later_of_entry[order] = self.later
        self.inline_of_entry = np.zeros(self.nnz, bool)
        self.inline_of_entry[order] = self.inline_eligible
        self.Bc = Bc

    def window(self, blk: int):
        """per sorted entry, for a workgroup of blk entries: (left side leaves the LDS window, right side leaves it); either sends the
        entry to run_bounds.  A run that only TOUCHES the window's first or last key counts as leaving: the kernel cannot tell."""
        x0 = (np.arange(self.nnz) // blk) * blk
        left = (x0 > EMIT_HALO) & (self.lo <= x0 - EMIT_HALO)
        right = (self.hi >= x0 + blk + EMIT_HALO) & (x0 + blk + EMIT_HALO < self.nnz)
        return left, right

    def bisects(self):
        """per sorted entry, were it handed to run_bounds: (left side bisects, right side bisects)"""
        x = np.arange(self.nnz)
        return x - self.lo > LINEAR_STEPS, self.hi - (x + 1) > LINEAR_STEPS

    def chunks(self, row: int, inline: bool = False) -> list:
        """k_layout_compact_products on the row's entries, 64 at a time: (live entries, T, 'fast' | 'search' | 'none')"""
        cnt = self.later_of_entry[self.Bc[row]:self.Bc[row + 1]]
        out = []
        for e0 in range(0, len(cnt), CHUNK):
            c = cnt[e0:e0 + CHUNK]
            live, T = int((c != 0).sum()), int(c.sum())
            out.append((live, T, "none" if T == 0 else "fast" if live == T else "search"))
        return out

    def rounds(self, row: int, compacted: bool = True) -> list:
        """k_layout_rowlists on the row's entries (the live ones of a compacted B'), 1,024 at a time: (tot, nround, L)"""
        cnt = self.later_of_entry[self.Bc[row]:self.Bc[row + 1]]
        if compacted:
            cnt = cnt[cnt != 0]
        out = []
        for jb in range(0, len(cnt), ROWLIST_BLOCK):
            c = cnt[jb:jb + ROWLIST_BLOCK]
            tot, nround = int(c.sum()), len(c)
            out.append((tot, nround, 1 if tot <= 2 * nround else 4 if tot <= 12 * nround else 16))
        return out

    def live_entries(self) -> int:
        own = np.repeat(np.arange(self.nreads) % self.stride == self.first, np.diff(self.Bc))
        return int(((self.later_of_entry != 0) & own).sum())

    def products(self) -> int:
        own = np.repeat(np.arange(self.nreads) % self.stride == self.first, np.diff(self.Bc))
        return int(self.later_of_entry[own].sum())
