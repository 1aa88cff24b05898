"""Read sets built for the EDGES of operand assembly (assemble.hpp, slotorder.hpp; bella_hip.hip: assemble_rows_device, build_layout):
table classes and load 1.0, duplicates and the insertion rounds, probe chains that wrap, the persistent loop of the global class, the
LDS window of k_layout_emit and run_bounds, palindromes, the degree limit, the place pass with and without its radix pass, 64-entry
chunks of the compaction and 1,024-entry rounds of the row lists.  Test tooling: nothing here is used by the product.

A set is reads + explicit tuples (kmer, read, pos) + the geometry it was built for (`design`), read back from
bella_testkit/assemble_mirror.py -- a builder raises if the mirror does not find what the set is for.

Two rules:
    ids follow the sequences: every tuple is laid down with a DESIGNED KEY (which k-mer the builder means it to be), and finish() checks
    that two tuples carry the same key if and only if the bases at their positions are the same canonical k-mer (a chance collision of
    random bases raises).  Shared k-mers are the same stretch, or its reverse complement, planted in several reads;
    ids are labels: keys get their ids from the builder -- by default in key order, or steered (`ids`) to choose hash homes: ids that
    differ by multiples of ht share the home slot key * 107 & (ht - 1); ids for a home of hash_range are found by search."""
from __future__ import annotations

import numpy as np

from . import assemble_mirror as M
from . import synth

K = 17
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def revcomp(b: np.ndarray) -> np.ndarray:
    return _COMP[b[::-1]]


class Case:
    """name, family, k, seqs, rs, nkmers, tk / tr / tp (grouped by read), design: what the mirror found in it"""

    def rows(self) -> dict:
        if getattr(self, "_rows", None) is None:
            self._rows = M.rows_geometry(self.rs.nreads, self.tk, self.tr)
        return self._rows

    def pal_of_kmer(self) -> np.ndarray:
        """per k-mer id: the k-mer is its own reverse complement (from the bases of an occurrence)"""
        pal = np.zeros(self.nkmers, bool)
        pal[self.tk] = self.t_pal
        return pal

    def layout(self, B, first: int = 0, stride: int = 1) -> M.LayoutGeometry:
        """B = (colptr, rowids, values) of the oracle"""
        return M.LayoutGeometry(B[0], B[1], self.nkmers, self.pal_of_kmer(), first, stride)


class Builder:
    """reads as lists of segments (bases, offsets of tuples inside, their designed keys)"""

    def __init__(self, k: int, seed: int):
        self.k, self.rng = k, np.random.default_rng(seed)
        self.reads, self.nkeys = [], 0

    def keys(self, m: int) -> np.ndarray:
        self.nkeys += m
        return np.arange(self.nkeys - m, self.nkeys, dtype=np.int64)

    def bases(self, n: int) -> np.ndarray:
        return synth.BASES[self.rng.integers(0, 4, size=n, dtype=np.uint8)]

    def stretch(self, m: int):
        """m consecutive fresh k-mers: (bases[m + k - 1], keys[m])"""
        return self.bases(m + self.k - 1), self.keys(m)

    def seg(self, bases, keys, rc: bool = False):
        """a stretch as a segment, every k-mer a tuple; rc: the other strand, positions mirrored"""
        m = len(keys)
        if rc:
            return revcomp(bases), np.arange(m)[::-1].copy(), np.asarray(keys)[::-1].copy()       # (tuples stay in position order)
        return bases, np.arange(m), np.asarray(keys)

    def unit(self, bases, keys, j: int, rc: bool = False):
        """the single k-mer j of a stretch as a segment of k bases"""
        return self.seg(bases[j:j + self.k], keys[j:j + 1], rc)

    def read(self, segs) -> int:
        """append a read; returns its id"""
        self.reads.append(segs)
        return len(self.reads) - 1

    def filler(self, n: int = 40):
        return [(self.bases(n), np.zeros(0, np.int64), np.zeros(0, np.int64))]

    def finish(self, name: str, family: str, ids=None, nkmers=None, design=None) -> Case:
        k = self.k
        seqs, tr, tp, tkey, fwl, rcl = [], [], [], [], [], []
        for r, segs in enumerate(self.reads):
            start, pos, key = 0, [], []
            for b, off, ky in segs:
                pos.append(start + np.asarray(off, np.int64))
                key.append(np.asarray(ky, np.int64))
                start += len(b)
            s = np.concatenate([b for b, _, _ in segs]).tobytes()
            assert len(s) < 32768
            seqs.append(s)
            pos, key = np.concatenate(pos), np.concatenate(key)
            if len(pos):
                fw, rc = M.kmer_codes(s, k)
                fwl.append(fw[pos]); rcl.append(rc[pos])
                tr.append(np.full(len(pos), r)); tp.append(pos); tkey.append(key)
        c = Case()
        c.name, c.family, c.k, c.seqs = name, family, k, seqs
        c.rs = synth.readset_from_seqs(seqs)
        if not tr:
            c.tk, c.tr, c.tp = np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint16)
            c.t_pal, c.t_canon, c.t_key, c.nkmers, c.design = np.zeros(0, bool), np.zeros(0, np.uint64), np.zeros(0, np.int64), nkmers or 1, design or {}
            c.t_ori = np.zeros(0, bool)
            return c
        tr, tp, tkey, fw, rc = (np.concatenate(x) for x in (tr, tp, tkey, fwl, rcl))
        canon = np.minimum(fw, rc)
        check_consistent(tkey, canon)
        # ids: steered keys first, the others take the smallest free ids in key order
        label = np.full(self.nkeys, -1, np.int64)
        for ky, i in (ids or {}).items():
            label[ky] = i
        steered = label[label >= 0]
        assert len(np.unique(steered)) == len(steered), "two keys steered to one id"
        rest = np.flatnonzero(label < 0)
        label[rest] = np.setdiff1d(np.arange(self.nkeys), steered)[:len(rest)]
        tk = label[tkey]
        c.nkmers = int(tk.max()) + 1 if nkmers is None else nkmers
        assert int(tk.max()) < c.nkmers < 2 ** 32 - 16 and int(tp.max()) < 65536
        c.tk, c.tr, c.tp = tk.astype(np.uint32), tr.astype(np.uint32), tp.astype(np.uint16)
        c.t_pal, c.t_canon, c.t_key, c.t_ori = fw == rc, canon, tkey, fw > rc
        c.design = design or {}
        return c


def check_consistent(key, canon) -> None:
    """same designed key <=> same canonical k-mer at the positions"""
    nk, nc = len(np.unique(key)), len(np.unique(canon))
    pairs = len(np.unique(np.stack([key.astype(np.uint64), canon]), axis=1).T)
    if not (nk == nc == pairs):
        raise ValueError("designed keys and canonical k-mers disagree (a chance collision?): %d keys, %d k-mers, %d pairs" % (nk, nc, pairs))


def inv107(ht: int) -> int:
    return pow(107, -1, ht)


def id_for_home(home: int, ht: int, used: set, base: int = 0) -> int:
    """the smallest unused id >= base whose slot-table home in a table of ht slots is `home`"""
    i = (inv107(ht) * home) % ht
    i += ((base - i + ht - 1) // ht) * ht if base > i else 0
    while i in used:
        i += ht
    used.add(i)
    assert M.slot_home(i, ht) == home
    return i


def need(cond, what: str) -> None:
    if not cond:
        raise AssertionError("the mirror does not find what the set is for: " + what)


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
ROW_SIZES = (1, 15, 16, 17, 96, 97, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)


def row_classes() -> Case:
    """one read per size of ROW_SIZES, 70 more small ones, empty reads first, last and in between, in shuffled order"""
    b = Builder(K, 1)
    sizes = list(ROW_SIZES) + [int(x) for x in b.rng.integers(18, 90, size=70)] + [0, 0, 0]
    order = b.rng.permutation(len(sizes))
    sizes = [0] + [sizes[x] for x in order] + [0]
    for n in sizes:
        b.read(b.filler() if n == 0 else [b.seg(*b.stretch(n))])
    c = b.finish("row_classes", "row_classes")
    g = c.rows()
    got = sorted(x.n for x in g.values())
    need(got == sorted(s for s in sizes if s), "sizes")
    need(0 not in g and c.rs.nreads - 1 not in g and c.rs.nreads % 256 != 0, "empty first / last read, ragged read count")
    need(M.class_counts(g)[0] >= 65 and min(M.class_counts(g)) >= 1, "65 reads of one class, every class present")
    for w in range(0, c.rs.nreads, 64):                      # some wavefront of k_asm_classify sees several classes and an empty read
        cl = {g[r].cls if r in g else -1 for r in range(w, min(w + 64, c.rs.nreads))}
        if len(cl) >= 4:
            break
    else:
        need(False, "a wavefront with mixed classes")
    need(not any(x.dup for x in g.values()), "no duplicates")
    c.design = dict(sizes=sizes, full=[x.n for x in g.values() if x.n == x.ht])
    return c


def _dup_read(b: Builder, n: int, dups) -> list:
    """a stretch of n k-mers followed by copies of single k-mers of it: dups = [index into the stretch, ...] in tuple order, so that the
    read has n + len(dups) tuples; every copy sits at a position of its own"""
    bases, keys = b.stretch(n)
    return [b.seg(bases, keys)] + [b.unit(bases, keys, j, rc=bool(x & 1)) for x, j in enumerate(dups)]


def row_duplicates() -> Case:
    b = Builder(K, 2)
    names = {}

    def add(name, segs):
        names[name] = b.read(segs)
    add("twice", _dup_read(b, 40, [7]))
    add("thrice", _dup_read(b, 40, [7, 7]))                          # first = 7, middle = 40, last = 41: the middle one must not win
    add("first-by-last", _dup_read(b, 50, [0]))
    # every tuple the same k-mer: a homopolymer read (d = 1)
    key = b.keys(1)
    add("all-same", [(np.full(60 + K - 1, ord("A"), np.uint8), np.arange(60), np.repeat(key, 60))])
    # ht = 128: one round up to d = 96, two from d = 97 on; n == ht in both
    add("one-round", _dup_read(b, 96, list(range(0, 64, 2))))        # n = 128, d = 96
    add("two-rounds", _dup_read(b, 97, list(range(0, 62, 2))))       # n = 128, d = 97
    add("full-1024", _dup_read(b, 1000, list(range(5, 29))))         # n = 1024 == ht, d = 1000: four rounds
    # occurrences on both sides of tuple index kPre * BLK = 4096 (class 3 and the global class: the smaller classes hold every tuple
    # in registers), and both before / both after it
    s, ky = b.stretch(5000)
    add("prefetch-3", [b.seg(s[:3000 + K - 1], ky[:3000]), b.unit(s, ky, 10), b.unit(s, ky, 11), b.seg(s[3000:], ky[3000:]), b.unit(s, ky, 10, True),
                       b.unit(s, ky, 4500), b.unit(s, ky, 20), b.unit(s, ky, 4999)])
    s, ky = b.stretch(9000)
    add("prefetch-global", [b.seg(s[:4000 + K - 1], ky[:4000]), b.unit(s, ky, 3999), b.seg(s[4000:], ky[4000:]), b.unit(s, ky, 0, True),
                            b.unit(s, ky, 8999), b.unit(s, ky, 4096), b.unit(s, ky, 4095)])
    add("prefetch-1", _dup_read(b, 2000, [0, 1999, 1000]))           # classes 1 and 2: duplicates, every tuple in registers
    add("prefetch-2", _dup_read(b, 4000, [0, 3999, 2000]))
    c = b.finish("row_duplicates", "row_duplicates")
    g = c.rows()
    need(all(x.dup for x in g.values()), "every read has a duplicate")
    need(g[names["all-same"]].d == 1, "d = 1")
    need((g[names["one-round"]].n, g[names["one-round"]].d, g[names["one-round"]].rounds) == (128, 96, 1), "dup, one round")
    need((g[names["two-rounds"]].n, g[names["two-rounds"]].d, g[names["two-rounds"]].rounds) == (128, 97, 2), "dup, two rounds")
    need(g[names["full-1024"]].n == 1024 and g[names["full-1024"]].rounds >= 3, "dup at load 1.0")
    for nm, cls in (("prefetch-3", 3), ("prefetch-global", 4), ("prefetch-1", 1), ("prefetch-2", 2)):
        x = g[names[nm]]
        need(x.cls == cls and x.beyond_prefetch == (cls >= 3), nm)
        if cls >= 3:
            lim = M.K_PRE * x.blk
            sides = {(x.first[km] < lim, x.last[km] < lim) for km in x.first if x.first[km] != x.last[km]}
            need(sides == {(True, True), (True, False), (False, False)}, nm + ": duplicates on both sides of the prefetch")
    # last-wins is visible: the occurrences of a duplicate have different positions
    starts = np.searchsorted(c.tr, np.arange(c.rs.nreads + 1))
    for r, x in g.items():
        pos = c.tp[starts[r]:starts[r + 1]]
        need(all(pos[x.first[km]] != pos[x.last[km]] for km in x.first if x.first[km] != x.last[km]), "positions differ per occurrence")
    c.design = dict(names=names)
    return c


def _search_dedup_ids(KS: int, slot_lo: int, count: int, used: set, base: int) -> list:
    """`count` unused ids >= base whose de-duplication home (hash_range) is one of the slots slot_lo .. KS - 1"""
    out, i = [], base
    while len(out) < count:
        if i not in used and M.hash_range(i, KS) >= slot_lo:
            out.append(i)
            used.add(i)
        i += 1
    return out


def row_probes() -> Case:
    b = Builder(K, 3)
    ids, used, names = {}, set(), {}
    base = [0]

    def steered(name, n, homes=None, ht=None, dedup_tail=0):
        """a read of n private k-mers; tuple t's id has slot-table home homes[t] (None: any); the first dedup_tail tuples instead get ids
        whose de-duplication home lies in the last two slots of the table"""
        s, ky = b.stretch(n)
        g_ht = M.pow2_at_least(16, n)
        assert ht is None or ht == g_ht
        KS = M.asm_dedup_slots(g_ht if M.asm_class_of(g_ht) < 4 else n)
        tail = _search_dedup_ids(KS, KS - 2, dedup_tail, used, base[0]) if dedup_tail else []
        for t in range(n):
            if t < dedup_tail:
                ids[int(ky[t])] = tail[t]
            elif homes is not None:
                ids[int(ky[t])] = id_for_home(homes[t], g_ht, used, base[0])
        names[name] = b.read([b.seg(s, ky)])
        base[0] = max(used) + 1 if used else 0
    for ht, n in ((16, 16), (128, 128), (1024, 1024)):
        steered("one-home-%d" % ht, n, [5] * n, ht)                                   # every k-mer on one home slot, load 1.0
        steered("tail-%d" % ht, n, [ht - 1 - (t % 4) for t in range(n)], ht)          # homes in the last four slots: the chains wrap to slot 0
        steered("dedup-wrap-%d" % ht, n - 3, None, ht, dedup_tail=6)
    # late rounds whose free slots lie only BEFORE the homes: build_next_free wraps (ht = 128 and 1024: ht = 16 has one round)
    steered("nf-wrap-128", 128, [120] * 128, 128)
    steered("nf-wrap-1024", 1024, [1016] * 1024, 1024)
    # the global class: homes in the last 64 slots of 16,384, and a chain over the end of the de-duplication table
    steered("global", 16000, [16384 - 1 - (t % 64) for t in range(16000)], 16384, dedup_tail=6)
    c = b.finish("row_probes", "row_probes", ids=ids)
    g = c.rows()
    for ht in (16, 128, 1024):
        need(len(g[names["one-home-%d" % ht]].slot_homes) == 1 and g[names["one-home-%d" % ht]].slot_chain == ht - 1, "one home")
        need(g[names["tail-%d" % ht]].slot_wraps, "slot chain wraps")
        need(g[names["dedup-wrap-%d" % ht]].dedup_wraps, "dedup chain wraps")
    need(g[names["nf-wrap-128"]].next_free_wraps and g[names["nf-wrap-1024"]].next_free_wraps, "next-free wraps")
    x = g[names["global"]]
    need(x.cls == 4 and x.slot_wraps and x.dedup_wraps and x.next_free_wraps, "global read: wraps")
    c.design = dict(names=names)
    return c


GLOBAL_READS = 130


def row_global() -> Case:
    """130 reads of the global class (more than kAsmGrid = 128: two workgroups take a second read) beside a few small ones.  The list
    k_asm_classify writes is ordered inside a wavefront and by arrival between wavefronts; the reads 0 .. 129 are three wavefronts'
    worth (64, 64, 2).  When the short wavefront arrives last, list places 128, 129 (second reads) are reads 128, 129 and places
    0, 1 are reads 0, 1 or 64, 65; when it arrives first the second reads are 62, 63 or 126, 127 after 128, 129.  The sizes are set so
    that in both orders one workgroup's second read has the smaller table and the other's the larger one.
    k = 31: among 1.1 M random 17-mers some seventy pairs would be the same k-mer by chance."""
    b = Builder(31, 4)
    n_of = {r: 8193 + (r % 7) for r in range(GLOBAL_READS)}
    big, small = 16385, 8193
    for r in (0, 64, 129, 62, 126):
        n_of[r] = big                                    # ht = 32,768
    for r in (1, 65, 128, 63, 127):
        n_of[r] = small                                  # ht = 16,384
    n_of[2], n_of[3] = 16384, 8193                       # n == ht
    dup_reads = (5, 70)
    for r in range(GLOBAL_READS):
        if r in dup_reads:
            b.read(_dup_read(b, n_of[r] - 3, [0, 5000, n_of[r] - 4]))
        else:
            b.read([b.seg(*b.stretch(n_of[r]))])
    for n in (0, 30, 3000, 0):
        b.read(b.filler() if n == 0 else [b.seg(*b.stretch(n))])
    c = b.finish("row_global", "row_global")
    g = c.rows()
    need(M.class_counts(g)[4] == GLOBAL_READS > M.ASM_GRID, "130 reads of the global class")
    need(sorted(M.global_schedule(g), reverse=True)[:3] == [2, 2, 1], "two workgroups take a second read")
    ns = {x.n for x in g.values()}
    need({8193, 16384, 16385} <= ns, "sizes")
    need(g[128].ht < g[0].ht and g[128].ht < g[64].ht and g[129].ht > g[1].ht and g[129].ht > g[65].ht, "second read smaller / larger (short wavefront last)")
    need(g[62].ht > g[128].ht and g[126].ht > g[128].ht and g[63].ht < g[129].ht and g[127].ht < g[129].ht, "second read larger / smaller (short wavefront first)")
    need(sum(1 for r in range(GLOBAL_READS) if g[r].dup) == 2, "two reads with duplicates")
    c.design = dict(tuples=len(c.tk))
    return c


def row_limits() -> dict:
    """'max': one short read with 65,535 tuples (its ~100 positions over and over); 'over': 65,536 of them (status bit 16);
    'order': read ids that decrease (status bit 8)"""
    out = {}
    for name, n in (("max", 65535), ("over", 65536)):
        b = Builder(K, 5)
        b.read(b.filler())
        s, ky = b.stretch(100)
        t = np.arange(n) % 100
        b.read([(s, t, ky[t])])
        b.read([b.seg(*b.stretch(20))])
        c = b.finish("row_limits_" + name, "row_limits")
        if name == "max":
            g = c.rows()[1]
            need((g.n, g.ht, g.d, g.cls, g.dup) == (65535, 65536, 100, 4, True), "65,535 tuples")
        out[name] = c
    b = Builder(K, 6)
    for n in (10, 20, 30):
        b.read([b.seg(*b.stretch(n))])
    c = b.finish("row_limits_order", "row_limits")
    c.tk, c.tr, c.tp = c.tk[::-1].copy(), c.tr[::-1].copy(), c.tp[::-1].copy()
    out["order"] = c
    return out


# ---- layouts: sets given by the degree of every k-mer -------------------------------------------------------------------------------
def from_degrees(name: str, family: str, degree_of_id: dict, nreads: int, seed: int, k: int = K, nkmers=None, pal=()) -> Case:
    """degree_of_id: {k-mer id: reads that hold it}.  Every k-mer is one k-base unit planted in that many reads chosen at random (so
    the sharers are not in planting order), half of the occurrences as the reverse complement; a read is the shuffled concatenation of
    its units.  pal: ids whose k-mer is a palindrome (even k)."""
    b = Builder(k, seed)
    rng = b.rng
    per_read = [[] for _ in range(nreads)]
    ids = {}
    for i, dg in degree_of_id.items():
        if dg == 0:
            continue
        assert dg <= nreads
        if i in pal:
            half = b.bases(k // 2)
            bases, key = np.concatenate([half, revcomp(half)]), b.keys(1)
        else:
            bases, key = b.stretch(1)
        ids[int(key[0])] = i
        for r in rng.choice(nreads, size=dg, replace=False) if dg < nreads else np.arange(nreads):
            per_read[int(r)].append(b.seg(bases, key, rc=bool(rng.integers(0, 2))))
    for r in range(nreads):
        segs = per_read[r]
        rng.shuffle(segs)
        b.read(segs if segs else b.filler())
    return b.finish(name, family, ids=ids, nkmers=nkmers)


RUN_DEGREES = (1, 2, 3, 16, 17, 18, 33, 34, 64, 65, 300, 1100)


def runs_plan() -> list:
    """the degree of every k-mer id in id order = the runs of the sort in order.  Events at the multiples of 1,024 (the first entry of a
    workgroup of 256 and of 1,024 entries) and at some multiples of 256 only: runs that begin at a workgroup's first entry, 31, 32 and 33
    entries before it, that end 31, 32 and 33 past a workgroup's last entry; the first and the last run of the sort are long."""
    events = {}                                                        # start offset -> degree

    def put(lo, hi):
        events[lo] = hi - lo
    for B, kind in ((1024, "begin"), (2048, "l32"), (3072, "l33"), (4096, "r32"), (5120, "r33"), (6144, "l31"), (7168, "r31"),
                    (256, "begin"), (512, "l32"), (768, "l33"), (1280, "r32"), (1536, "r33")):
        if kind == "begin":
            put(B, B + 3)
        elif kind[0] == "l":
            put(B - int(kind[1:]), B + 2)
        else:
            put(B - 2, B + int(kind[1:]))
    put(0, 18)                                                         # the first run of the sort
    put(8192, 8192 + 300)                                              # longer than a workgroup of 256 and both halos
    put(8600, 8600 + 1100)                                             # longer than a workgroup of 1,024
    put(9800, 9800 + 65)
    put(9900, 9900 + 64)                                               # the last run: ends at nnz
    end = 9964
    plan, x = [], 0
    small = [1, 2, 3, 16, 17, 1, 1, 33, 1, 2, 34, 1, 1, 2, 1, 3]       # what fills the gaps, as far as it fits
    f = 0
    for lo in sorted(events):
        while x < lo:
            dg = small[f % len(small)]
            f += 1
            if x + dg > lo:
                dg = 1
            plan.append(dg)
            x += dg
        assert x == lo
        plan.append(events[lo])
        x += events[lo]
    assert x == end
    return plan


def runs() -> Case:
    plan = runs_plan()
    c = from_degrees("runs", "runs", dict(enumerate(plan)), 1200, seed=7)
    c.design = dict(plan=plan, nnz=sum(plan))
    return c


def runs_census(L: M.LayoutGeometry) -> dict:
    """what the mirror finds in a layout, per workgroup size"""
    out = {}
    x = np.arange(L.nnz)
    for blk in M.EMIT_BLOCKS:
        x0 = (x // blk) * blk
        left, right = L.window(blk)
        bl, br = L.bisects()
        glob = left | right
        last_wg = x0 == ((L.nnz - 1) // blk) * blk
        out[blk] = {
            "begins-at-first-entry": bool(((L.lo == x0) & (x0 > 0) & (L.degree > 1)).any()),
            "begins-31-before": bool(((L.lo == x0 - 31) & (x >= x0) & ~left).any()),
            "begins-32-before": bool(((L.lo == x0 - 32) & left).any()),
            "begins-33-before": bool(((L.lo == x0 - 33) & left).any()),
            "ends-31-past": bool(((L.hi == x0 + blk + 31) & ~right).any()),
            "ends-32-past": bool(((L.hi == x0 + blk + 32) & right).any()),
            "ends-33-past": bool(((L.hi == x0 + blk + 33) & right).any()),
            "first-workgroup-long-run": bool(((x0 == 0) & (L.lo == 0) & (L.degree > 16)).any()),
            "last-workgroup-run-to-the-end": bool((last_wg & (L.hi == L.nnz) & (L.degree > 32)).any()),
            # an entry handed to run_bounds: each side ends inside its 16 linear steps (exactly 16: the last that does) or bisects
            "run-bounds-left-16-steps": bool((glob & (x - L.lo == M.LINEAR_STEPS)).any()),
            "run-bounds-left-bisects-at-17": bool((glob & (x - L.lo == M.LINEAR_STEPS + 1)).any()),
            "run-bounds-right-16-steps": bool((glob & (L.hi - (x + 1) == M.LINEAR_STEPS)).any()),
            "run-bounds-right-bisects-at-17": bool((glob & (L.hi - (x + 1) == M.LINEAR_STEPS + 1)).any()),
            "run-bounds-both-bisect": bool((glob & bl & br).any()),
            "run-bounds-left-0-steps": bool((glob & (x == L.lo)).any()),
            "run-bounds-right-0-steps": bool((glob & (x + 1 == L.hi)).any()),
            "run-longer-than-window": bool((L.degree > blk + 2 * M.EMIT_HALO).any()),
        }
    return out


def palindromes() -> Case:
    """k = 16: palindromic k-mers of degree 1, 2, 3 and 40 next to plain ones of degree 2 (both relative orientations occur among the 12
    of them: from_degrees plants either strand at random; the census checks it)"""
    deg = {0: 1, 1: 2, 2: 3, 3: 40}
    for i in range(4, 16):
        deg[i] = 2
    deg[16], deg[17] = 2, 5                                            # two more palindromes
    c = from_degrees("palindromes", "palindromes", deg, 60, seed=8, k=16, pal=(0, 1, 2, 3, 16, 17))
    pal = c.pal_of_kmer()
    need(sorted(np.flatnonzero(pal)) == [0, 1, 2, 3, 16, 17], "the palindromes")
    c.design = dict(degrees=deg)
    return c


def palindromes_k2() -> Case:
    """k = 2: every position of five random reads; the key of a tuple IS its canonical 2-mer (AT, TA, CG, GC are palindromes)"""
    b = Builder(2, 9)
    canon_key = {}
    for r in range(5):
        s = b.bases(14)
        fw, rc = M.kmer_codes(s.tobytes(), 2)
        keys = []
        for cc in np.minimum(fw, rc):
            if int(cc) not in canon_key:
                canon_key[int(cc)] = int(b.keys(1)[0])
            keys.append(canon_key[int(cc)])
        b.read([(s, np.arange(13), np.asarray(keys))])
    c = b.finish("palindromes_k2", "palindromes")
    need(c.t_pal.any() and not c.t_pal.all(), "palindromes and plain 2-mers")
    return c


def degree_limit(nshare: int) -> Case:
    """one k-mer in `nshare` short reads (16,383: the largest degree a B' entry holds; 16,384: status bit 64), and a rest: three k-mers of
    degree 2, 3 and 5"""
    deg = {0: 2, 1: nshare, 2: 3, 3: 5}
    c = from_degrees("degree_%d" % nshare, "degree_limit", deg, nshare + 4, seed=10)
    c.design = dict(flops=sum(d * (d - 1) // 2 for d in deg.values()), nshare=nshare)
    return c


SIZES = ((1, 2), (255, 3), (256, 256), (257, 257), (2048, 4096), (4096, 4097), (4097, 1 << 20), (300, (1 << 20) + 1),
         (13000, 4096))               # (a third of 13,000 is more than 4,096: the place pass of a PARTITION sorts)


def sizes(nnz: int, nkmers: int, nreads=None, name=None) -> Case:
    """a matrix of nnz nonzeros over ids 0 .. nkmers - 1 with the largest id in use"""
    rng = np.random.default_rng(nnz)
    nuse = min(nkmers, max(1, nnz // 2))
    if nuse == 1:
        use = np.asarray([nkmers - 1])
    else:
        mid = rng.choice(nkmers - 2, size=nuse - 2, replace=False) + 1 if nuse > 2 else np.zeros(0, np.int64)
        use = np.sort(np.concatenate([[0, nkmers - 1], mid]))
    deg = np.full(len(use), nnz // len(use))
    deg[:nnz - int(deg.sum())] += 1
    nreads = nreads or max(int(deg.max()) + 3, 50)
    c = from_degrees(name or "sizes_%d_%d" % (nnz, nkmers), "sizes", {int(i): int(d) for i, d in zip(use, deg)}, nreads, seed=11 + nnz, nkmers=nkmers)
    need(len(c.tk) == nnz and int(c.tk.max()) == nkmers - 1, "nnz and the largest id")
    c.design = dict(nnz=nnz, nkmers=nkmers)
    return c


def sizes_sparse() -> Case:
    """fewer nonzeros than reads"""
    return sizes(5, 9, nreads=3000, name="sizes_sparse")


# ---- rows of B' designed entry by entry --------------------------------------------------------------------------------------------
def hub_set(name: str, family: str, rows: list, npartners: int, seed: int) -> Case:
    """rows: per hub read the later-read count of every entry IN ROW ORDER.  Hub h is read h, a stretch of len(rows[h]) consecutive
    k-mers; entry j's id is steered to home slot j of the hub's table (distinct homes: the slot order is the home order); its k-mer is
    planted in rows[h][j] of the `npartners` partner reads that follow the hubs."""
    b = Builder(K, seed)
    rng = b.rng
    ids, used = {}, set()
    nh = len(rows)
    partner = [[] for _ in range(npartners)]
    for h, cnts in enumerate(rows):
        n = len(cnts)
        ht = M.pow2_at_least(16, n)
        s, ky = b.stretch(n)
        perm = rng.permutation(n)                                      # tuple order is not row order
        for j in range(n):
            ids[int(ky[perm[j]])] = id_for_home(j, ht, used)
        b.read([b.seg(s, ky)])
        for j in range(n):
            for p in rng.choice(npartners, size=cnts[j], replace=False):
                partner[int(p)].append(b.unit(s, ky, int(perm[j]), rc=bool(rng.integers(0, 2))))
    for p in range(npartners):
        rng.shuffle(partner[p])
        b.read(partner[p] if partner[p] else b.filler())
    c = b.finish(name, family, ids=ids)
    c.design = dict(rows=rows, hubs=nh)
    return c


def chunks() -> Case:
    one, dead = [1] * 64, [0] * 64
    rows = [
        dead + one,                                                    # a chunk with no live entry, then the fast path
        [1] * 30 + [2] + [1] * 33,                                     # one entry with two later reads among 63 with one: search
        [1] * 10 + [70] + [0] * 53,                                    # T > 64
        [0] * 63 + [1] + [1] + [0] * 63,                               # live entries as the last of a chunk and the first of the next
        [1, 0] * 32,                                                   # exactly 64 entries
        [0, 2] * 32 + [3],                                             # 65 entries
        [1] * 5, [0] * 7, [2] * 5,                                     # a row with no live entry between two that have some
    ]
    c = hub_set("chunks", "chunks", rows, 80, seed=12)
    return c


def rowlists() -> Case:
    rows = [
        [2] * 10,                                                      # tot == 2 nround: L = 1
        [2] * 9 + [3],                                                 # 2 nround + 1: L = 4
        [12] * 10,                                                     # 12 nround: L = 4
        [12] * 9 + [13],                                               # 12 nround + 1: L = 16
        [1, 1, 5, 5, 1, 5, 5, 5, 1, 5],                                # inline entries inside an L = 4 round
        [1, 30, 1, 30, 30, 1, 30, 30, 30, 30],                         # ... inside an L = 16 round
        [2] * 1024 + [1],                                              # 1,025 entries: a full round with tot == 2 nround, then one entry
        [1] * 1000 + [3] * 24 + [3] * 1024 + [2],                      # 2,049 entries: three rounds (L = 1, 4, 1), `running` carries
    ]
    return hub_set("rowlists", "rowlists", rows, 80, seed=13)


def check_hub_rows(c: Case, L: M.LayoutGeometry) -> None:
    """the rows of the hubs hold the designed later-read counts in the designed order"""
    for h, cnts in enumerate(c.design["rows"]):
        got = L.later_of_entry[L.Bc[h]:L.Bc[h + 1]]
        need(len(got) == len(cnts) and np.array_equal(got, cnts), "%s: hub %d" % (c.name, h))


# ---- the families ----------------------------------------------------------------------------------------------------------------------
def _sizes_cases() -> dict:
    d = {"sizes_%d_%d" % (nnz, nk): (lambda nnz=nnz, nk=nk: sizes(nnz, nk)) for nnz, nk in SIZES}
    d["sizes_sparse"] = sizes_sparse
    return d


FAMILIES = {
    "row_classes": {"row_classes": row_classes},
    "row_duplicates": {"row_duplicates": row_duplicates},
    "row_probes": {"row_probes": row_probes},
    "row_global": {"row_global": row_global},
    "row_limits": {"row_limits_" + n: (lambda n=n: row_limits()[n]) for n in ("max", "over", "order")},
    "runs": {"runs": runs},
    "palindromes": {"palindromes": palindromes, "palindromes_k2": palindromes_k2},
    "degree_limit": {"degree_16383": lambda: degree_limit(16383), "degree_16384": lambda: degree_limit(16384)},
    "sizes": _sizes_cases(),
    "chunks": {"chunks": chunks},
    "rowlists": {"rowlists": rowlists},
}
ROW_FAMILIES = ("row_classes", "row_duplicates", "row_probes", "row_global")
LAYOUT_FAMILIES = ("runs", "palindromes", "sizes", "chunks", "rowlists")
ERRORS = {"row_limits_over": 16, "row_limits_order": 8, "degree_16384": 64}         # the status bit a case must raise
_made = {}


def case(name: str) -> Case:
    """the case of that name, built once and shared (read-only)"""
    if name not in _made:
        fam = next(f for f, d in FAMILIES.items() if name in d)
        c = FAMILIES[fam][name]()
        assert c.name == name and c.family == fam, (c.name, name)
        for a in (c.tk, c.tr, c.tp):
            a.setflags(write=False)
        _made[name] = c
    return _made[name]


def names(*families) -> list:
    return [n for f in families for n in FAMILIES[f]]


def census_rows(c: Case) -> set:
    """the row geometry the mirror finds in a case, as keys"""
    if c.name in ("row_limits_over", "row_limits_order"):
        return {c.name}
    g, out, nr = c.rows(), set(), c.rs.nreads
    starts = np.searchsorted(c.tr, np.arange(nr + 1))
    for r, x in g.items():
        out.add("class-%d" % x.cls)
        if not x.dup:
            out.add("n=%d" % x.n)
            if x.n == x.ht:
                out.add("load-1.0-ht=%d" % x.ht)
            if x.ht == 128:
                out.add("ht=128-rounds=%d" % x.rounds)
            if x.rounds > 2:
                out.add("several-rounds")
        if x.beyond_prefetch:
            out.add("beyond-prefetch-class-%d" % x.cls)
        if x.n == 65535:
            out.add("n=65535")
        if x.cls == 4:
            out.add("global-n=%d" % x.n)
        if len(x.slot_homes) == 1 and x.d == x.ht:
            out.add("one-home-ht=%d" % x.ht)
        if x.slot_wraps and x.d == x.ht:
            out.add("slot-chain-wraps-ht=%d" % x.ht)
        if x.dedup_wraps:
            out.add("dedup-chain-wraps-ht=%d" % x.ht)
        if x.next_free_wraps:
            out.add("next-free-wraps-ht=%d" % x.ht)
        if x.cls == 4 and x.slot_wraps and x.dedup_wraps and x.next_free_wraps:
            out.add("global-class-wraps")
        if x.dup:
            pos = c.tp[starts[r]:starts[r + 1]]
            km = c.tk[starts[r]:starts[r + 1]]
            cnt = np.unique(km, return_counts=True)[1]
            lim = M.K_PRE * x.blk
            out.add("dup")
            out.add("dup-class-%d" % x.cls)
            if 2 in cnt:
                out.add("dup-twice")
            if any(x.first[k] < t < x.last[k] and pos[t] != pos[x.first[k]] and pos[t] != pos[x.last[k]]
                   for t, k in enumerate(int(v) for v in km[:200])):
                out.add("dup-thrice-middle")
            if km[0] == km[-1]:
                out.add("dup-first-by-last")
            if x.d == 1:
                out.add("dup-d=1")
            out.add("dup-one-round" if x.rounds == 1 else "dup-several-rounds")
            if x.ht == 128 and x.n == 128:
                out.add("dup-ht=128-d=%d-rounds=%d" % (x.d, x.rounds))
            if x.n == x.ht:
                out.add("dup-load-1.0")
            if any(x.first[k] < lim <= x.last[k] for k in x.first):
                out.add("dup-across-prefetch-class-%d" % x.cls)
            if all(pos[x.first[k]] != pos[x.last[k]] for k in x.first if x.first[k] != x.last[k]):
                out.add("dup-positions-differ")
    cc = M.class_counts(g)
    if 0 not in g:
        out.add("empty-read-first")
    if nr - 1 not in g:
        out.add("empty-read-last")
    for r in range(1, nr - 1):
        if r not in g and r - 1 in g and r + 1 in g and g[r - 1].cls != g[r + 1].cls:
            out.add("empty-read-between-classes")
    if max(cc) >= 65 and sum(1 for v in cc if v) >= 2:
        out.add("65-reads-of-one-class-beside-others")
    for w in range(0, nr, 64):
        if len({g[r].cls for r in range(w, min(w + 64, nr)) if r in g}) >= 3:
            out.add("wavefront-with-mixed-classes")
    if nr % 256:
        out.add("ragged-read-count")
    if cc[4] > M.ASM_GRID:
        out.add("global-class-more-reads-than-workgroups")
        if sorted(M.global_schedule(g))[-2:] == [2, 2]:
            out.add("two-workgroups-take-a-second-read")
        # (k_asm_classify lists the reads wavefront by wavefront, in the order the wavefronts arrive; row_global explains the two orders)
        if all(r in g for r in (0, 1, 64, 65, 128, 129)) and g[128].ht < min(g[0].ht, g[64].ht) and g[129].ht > max(g[1].ht, g[65].ht):
            out.add("second-read-smaller-and-larger-table")
        if sum(1 for x in g.values() if x.cls == 4 and x.dup) == 2:
            out.add("global-class-two-reads-with-duplicates")
    return out


def census_layout(c: Case, B) -> set:
    """the layout geometry the mirror finds in a case (B: the oracle's rows), as keys"""
    L = c.layout(B)
    out = set()
    for blk, d in runs_census(L).items():
        out |= {"wg%d-%s" % (blk, key) for key, v in d.items() if v}
    for dg in np.unique(L.degree):
        out.add("degree=%d" % dg)
    pal, plain = L.pal, ~L.pal
    for dg in np.unique(L.degree[pal]):
        out.add("palindrome-degree=%d" % dg)
    if (pal & (L.rank + 2 == L.degree)).any() and not (pal & L.inline_eligible).any():
        out.add("palindrome-last-but-one-not-inline")
    # plain k-mers of degree 2: the two occurrences on the same strand / on different strands
    e_ori = {}
    for t in range(len(c.tk)):
        e_ori[(int(c.tr[t]), int(c.tk[t]))] = bool(c.t_ori[t])
    for x in np.flatnonzero(plain & (L.degree == 2) & (L.rank == 0)):
        a, b2 = e_ori[(int(L.sread[x]), int(L.skey[x]))], e_ori[(int(L.sread[x + 1]), int(L.skey[x]))]
        out.add("inline-same-strand" if a == b2 else "inline-opposite-strands")
    if c.k == 2:
        out.add("k=2")
    if L.nnz and c.t_ori.any() and not c.t_ori.all():
        out.add("both-strands-planted")
    out.add("nnz=%d" % L.nnz)
    out.add("place-pass-sorts" if L.place_sorts else "place-pass-plain")
    for stride_first in range(3):
        Lp = c.layout(B, stride_first, 3)
        out.add("partitioned-place-pass-sorts" if Lp.place_sorts else "partitioned-place-pass-plain")
    b = L.kbits
    if c.nkmers == 1 << b:
        out.add("nkmers=2^%d" % b)
    if c.nkmers == (1 << (b - 1)) + 1:
        out.add("nkmers=2^%d+1" % (b - 1))
    if L.nnz and int(L.skey[-1]) == c.nkmers - 1:
        out.add("largest-id-in-use")
    if L.nnz < c.rs.nreads:
        out.add("fewer-nonzeros-than-reads")
    if L.over_degree:
        out.add("degree-over-limit")
    live_rows = []
    for r in range(L.nreads):
        n = int(L.Bc[r + 1] - L.Bc[r])
        if not n:
            continue
        ch = L.chunks(r)
        cnt = L.later_of_entry[L.Bc[r]:L.Bc[r + 1]]
        for live, T, kind in ch:
            out.add("chunk-" + kind)
            if T > 64:
                out.add("chunk-more-than-64-products")
            if kind == "search" and live == 64 and T == 65:
                out.add("chunk-one-entry-with-2-among-63-with-1")
        if n > 64 and cnt[63] and cnt[64]:
            out.add("live-entry-last-of-chunk-and-first-of-next")
        if n in (64, 65):
            out.add("row-of-%d-entries" % n)
        live_rows.append(bool(cnt.any()))
        if live_rows[-3:] == [True, False, True]:
            out.add("dead-row-between-live-rows")
        rounds = L.rounds(r)
        if len([1 for v in cnt if v]) in (1025, 2049):
            out.add("row-of-%d-live-entries" % int((cnt != 0).sum()))
        if len(rounds) > 1 and len({L_ for _, _, L_ in rounds}) > 1:
            out.add("rounds-with-different-L")
        live_cnt = cnt[cnt != 0]
        for x, (tot, nround, L_) in enumerate(rounds):
            for m, nm in ((2, "2n"), (12, "12n")):
                if tot == m * nround:
                    out.add("round-tot=" + nm)
                if tot == m * nround + 1:
                    out.add("round-tot=" + nm + "+1")
            out.add("round-L=%d" % L_)
            if L_ > 1 and (live_cnt[x * M.ROWLIST_BLOCK:(x + 1) * M.ROWLIST_BLOCK] == 1).any():
                out.add("one-product-entries-in-L=%d-round" % L_)
    return out
