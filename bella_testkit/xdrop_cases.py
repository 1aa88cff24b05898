"""Read sets and seeds that put the X-drop kernels (xdrop.hpp, xdrop_packed.hpp, run_xdrop) where they can go wrong: an extension
that drops, ends or enters Phase 4 on a chosen side of a launch boundary of the sliced kernel; flanks around the 32-base rule, the
16-base blocks and the 32 / 48-base window tops of the sequence registers; reads at the front and the back of the packed array, at
chosen residues of 16, behind a read shorter than one block; every k and X the band arithmetic distinguishes; and more survivors
and more extensions than one batch was ever given.

Where an event has to sit on an exact step, the input is FOUND: a family of inputs (an identical or once-edited prefix before a tail
that never matches, or a template cut to length) runs through xdrop_mirror, and the first member whose trace has the event on the
wanted step is taken.  A family without such a member raises.  tests/test_xdrop_cases_cpu.py then checks every label against the
trace once more, with the mirror held against the oracle: the search is not trusted.

An extension is designed as the two sequences IT reads (`h`, `v`); embed() turns the design into a pair of reads for either side
of the seed and either strand: the right extension reads what follows the seed, the left one the prefixes back to front with the
seed first, and on the "c" strand the row is stored as the reverse complement of what the extension reads."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from . import synth
from . import xdrop_mirror as M

S = 512                                     # steps per launch of the sliced kernel (BELLA_XDROP_SLICE, checked by the CPU test)
SEED_DT = np.dtype([("rid", "<u4"), ("cid", "<u4"), ("seedH", "<u2"), ("seedV", "<u2")])
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
SIDES = ("left", "right")
STRANDS = ("n", "c")


def rc(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def rnd(rng, n: int) -> bytes:
    return synth.BASES[rng.integers(0, 4, int(n))].tobytes()


@dataclasses.dataclass
class CaseSet:
    name: str
    k: int
    X: int
    seqs: list = dataclasses.field(default_factory=list)
    seeds: list = dataclasses.field(default_factory=list)          # (rid, cid, i, j)
    labels: list = dataclasses.field(default_factory=list)         # one dict per seed
    err: float = 0.15                                              # the error rate the threshold of `passed` is made from

    @property
    def rs(self):
        return synth.readset_from_seqs(self.seqs)

    def seed_array(self):
        sd = np.zeros(len(self.seeds), SEED_DT)
        for t, q in enumerate(self.seeds):
            sd[t] = q
        return sd

    def add_pair(self, row, col, i, j, **label):
        self.seqs += [row, col]
        self.seeds.append((len(self.seqs) - 2, len(self.seqs) - 1, i, j))
        self.labels.append(label)


def embed(rng, h: bytes, v: bytes, side: str, strand: str, k: int, oh: bytes = b"", ov: bytes = b""):
    """-> (row, col, i, j).  (h, v): what the extension of `side` reads; (oh, ov): what the other side's reads, after the seed.
    A left extension starts with the seed, so h[:k] == v[:k] there."""
    if side == "right":
        seed = rnd(rng, k)
        H, V, i, j = oh[::-1] + seed + h, ov[::-1] + seed + v, len(oh), len(ov)
    else:
        assert h[:k] == v[:k]
        seed = h[:k][::-1]
        H, V, i, j = h[::-1] + oh, v[::-1] + ov, len(h) - k, len(v) - k
    assert seed != rc(seed)
    return (rc(H), V, len(H) - i - k, j) if strand == "c" else (H, V, i, j)


def add_four_ways(cs: CaseSet, rng, h, v, **label):
    """the design on both sides of the seed and on both strands; the other side runs on a short unrelated pair or not at all"""
    for n, (side, strand) in enumerate((a, b) for a in SIDES for b in STRANDS):
        oh, ov = (rnd(rng, 40), rnd(rng, 44)) if n % 2 == 0 else (rnd(rng, 3), rnd(rng, 5))
        cs.add_pair(*embed(rng, h, v, side, strand, cs.k, oh, ov), side=side, strand=strand, **label)


# ---- the families the searches run over -----------------------------------------------------------------------------------------
def prefix_family(seed: int, plens, tail: int = 420):
    """an identical prefix of P bases (whole, or with one base of v taken out in its middle: the other parity of the step count),
    then tails that never match (A against C, C against A)"""
    rng = np.random.default_rng(seed)
    base = rnd(rng, max(plens) + 1)
    tails = ((b"A" * tail, b"C" * tail), (b"C" * tail, b"A" * tail))
    fam = []
    for P in plens:
        for edit in (0, 1):
            for th, tv in tails:
                pv = base[:P] if not edit else base[:P // 2] + base[P // 2 + 1:P + 1]
                fam.append((base[:P] + th, pv + tv))
                fam.append((pv + tv, base[:P] + th))                # (and with the two sequences exchanged: the band's other half)
    return fam


def planted_family(seed: int, plens, places, tail: int):
    """prefix_family's A against C, with two or three bases of the other tail's letter planted in one tail.  In a tail where nothing
    matches the band settles with its largest cell at 16 on the steps that carry the larger of the two interleaved diagonals, and the
    direction kept once nothing is positive is `right`, always; a few late matches off the diagonal leave it at `down`"""
    rng = np.random.default_rng(seed)
    base = rnd(rng, max(plens))
    fam = []
    for P in plens:
        for x in places:
            for w in (2, 3):
                th, tv = b"A" * tail, b"C" * x + b"A" * w + b"C" * (tail - x - w)
                fam.append((base[:P] + th, base[:P] + tv))
                fam.append((base[:P] + tv, base[:P] + th))
    return fam


def template_family(seed: int, lens, first: str, more: int = 60, spoiled=(0,)):
    """one template read by both: the sequence `first` has L bases, the other `more` further ones (whole, or with one base of the
    longer one taken out in the middle), so `first` ends first, on a step the length sets.  spoiled: the last q bases of the
    shorter one are A, which the template does not have, so the score is already falling when it ends"""
    rng = np.random.default_rng(seed)
    base = bytes(b"CGT"[x] for x in rng.integers(0, 3, max(lens) + more + 2))
    fam = []
    for L in lens:
        for edit, q in ((e, q) for e in (0, 1) for q in spoiled):
            short = base[:L - q] + b"A" * q
            long_ = base[:L + more] if not edit else base[:L // 2] + base[L // 2 + 1:L + more + 1]
            fam.append((short, long_) if first == "H" else (long_, short))
    return fam


def find(fam, X, want, what):
    """the first member of the family whose trace satisfies want(trace) -> (h, v)"""
    tr = M.extend_many([f[0] for f in fam], [f[1] for f in fam], X)
    for f, t in zip(fam, tr):
        if want(t):
            return f
    raise LookupError("no input for " + what)


def find_all(fam, X, wants):
    """{key: first member for want} for several targets over ONE run of the family"""
    tr = M.extend_many([f[0] for f in fam], [f[1] for f in fam], X)
    got = {}
    for key, want in wants.items():
        hit = [f for f, t in zip(fam, tr) if want(t)]
        if not hit:
            raise LookupError("no input for %r" % (key,))
        got[key] = hit[0]
    return got


# ---- launch boundary ------------------------------------------------------------------------------------------------------------
DROP_STEPS = (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1)
END_STEPS = (S - 28, S - 27, S - 14, S - 1, S, S + 1)


@functools.lru_cache(None)
def drop_set() -> CaseSet:
    """X-drop in Phase 2 on the last step of a launch, on the first of the next, and one later; at both boundaries"""
    cs = CaseSet("drop", 17, 7)
    rng = np.random.default_rng(7001)
    plens = list(range(S // 2 - 10, S // 2 + 25)) + list(range(S - 10, S + 25))
    got = find_all(prefix_family(7002, plens), cs.X,
                   {T: (lambda t, T=T: t["drop_step"] == T and t["drop_phase"] == 2) for T in DROP_STEPS})
    for T in DROP_STEPS:
        add_four_ways(cs, rng, *got[T], event="drop_p2", step=T)
    return cs


@functools.lru_cache(None)
def end_set() -> CaseSet:
    """Phase 2 ends -- H first, V first -- so that the 28 steps of Phase 4 lie before the boundary, end on it, straddle it, start on
    its last step or after it.  X = 60: Phase 4 runs all of its 28 steps"""
    cs = CaseSet("end", 17, 60)
    rng = np.random.default_rng(7011)
    lens = range(S // 2 + 5, S // 2 + 45)
    for first in "HV":
        got = find_all(template_family(7012, lens, first), cs.X,
                       {T: (lambda t, T=T: t["p2_end_step"] == T and t["p2_end_seq"] == first and t["p4_steps"] == M.TAIL) for T in END_STEPS})
        for T in END_STEPS:
            add_four_ways(cs, rng, *got[T], event="p2_end", step=T, seq=first)
    return cs


@functools.lru_cache(None)
def tail_drop_set() -> CaseSet:
    """Phase 2 ends before the boundary and the X-drop fires in Phase 4 after it: `it4` and the direction go through the state"""
    cs = CaseSet("taildrop", 17, 7)
    rng = np.random.default_rng(7021)
    for first in "HV":
        h, v = find(template_family(7022, range(S // 2 + 15, S // 2 + 40), first, spoiled=range(12, 40)), cs.X,
                    lambda t: t["drop_phase"] == 4 and t["p2_end_step"] < S <= t["drop_step"] and t["p2_end_seq"] == first, "tail drop " + first)
        add_four_ways(cs, rng, h, v, event="drop_p4", seq=first)
    return cs


@functools.lru_cache(None)
def kept_set(X: int) -> CaseSet:
    """the band's maximum is not positive on the last step of a launch and on the first of the next: the direction of the last
    positive step is kept (`upm` through the flags word), once to the right and once down"""
    cs = CaseSet("kept%d" % X, 17, X)
    rng = np.random.default_rng(7031 + X)
    fam = prefix_family(7032, range(150, 330, 2), tail=700) + planted_family(7033, range(160, 200, 3), range(40, 100, 3), tail=700)

    def want(d):
        return lambda t: (S - 1, d) in t["nonpos_steps"] and (S, d) in t["nonpos_steps"]
    got = find_all(fam, X, {d: want(d) for d in ("right", "down")})
    for d in ("right", "down"):
        add_four_ways(cs, rng, *got[d], event="kept", direction=d)
    return cs


@functools.lru_cache(None)
def early_set() -> CaseSet:
    """endings before the loop is under way: the X-drop inside Phase 1, on the very first step of Phase 2, a first step without a
    positive cell (`flagged`), and a clean pair that runs to the ends of both sequences.  k = 5: a left extension starts with the
    seed, and a first step without a positive cell needs a start that short"""
    cs = CaseSet("early", 5, 7)
    rng = np.random.default_rng(7041)
    gt = lambda n: bytes(b"GT"[x] for x in rng.integers(0, 2, n))
    fam = []
    for m in range(5, 32):                                          # m matching bases, r that match nothing anywhere, then matches
        for r in range(1, 30):
            pre, post = gt(m), gt(60)
            fam.append((pre + b"A" * r + post, pre + b"C" * r + post))
    got = find_all(fam, cs.X, {
        "p1_drop": lambda t: t["p1_drop"] and t["steps"] == 0,
        "first_step_drop": lambda t: not t["p1_drop"] and t["drop_step"] == 0,
        "flagged": lambda t: t["flagged"] == 1 and t["steps"] > 0,
        "clean": lambda t: t["drop_step"] is None and t["p4_steps"] == M.TAIL and not t["flagged"],
    })
    for ev, (h, v) in got.items():
        add_four_ways(cs, rng, h, v, event=ev)
    return cs


# ---- flank lengths --------------------------------------------------------------------------------------------------------------
FLANKS = (31, 32, 33, 47, 48, 49, 63, 64, 65)
PARTNERS = (32, 300)


@functools.lru_cache(None)
def flank_set() -> CaseSet:
    """every length around the 32-base rule, the 16-base block and the 32 / 48-base window tops, on H and on V, on either side of
    the seed, on both strands, against a partner flank of 32 and of 300; the other side of the seed always runs (80 bases), so a
    right extension that does not run shows the reference's write of `beg`"""
    cs = CaseSet("flank", 17, 7)
    rng = np.random.default_rng(7051)
    for a in FLANKS:
        for which in "HV":
            for partner in PARTNERS:
                for side in SIDES:
                    for strand in STRANDS:
                        t = rnd(rng, 330)
                        o = rnd(rng, 80)
                        h, v = (t[:a], t[:partner]) if which == "H" else (t[:partner], t[:a])
                        cs.add_pair(*embed(rng, h, v, side, strand, cs.k, o, o), event="flank", side=side, strand=strand, which=which,
                                    length=a, partner=partner)
    return cs


# ---- place in the packed array --------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def place_set(total_mod: int) -> CaseSet:
    """Windows of one template, forward or as reverse complements, so that every extension runs on identical bases to an END of the
    window -- which lies at base 0 of the packed array, at the array's last base (with the total = total_mod mod 16), at a read
    start = 0, 1, 15 mod 16, or right behind a read shorter than a block.  Each window is H and V, on both strands, against the
    long window that contains it; and two pairs of a read with itself."""
    k = 17
    cs = CaseSet("place%d" % total_mod, k, 7)
    rng = np.random.default_rng(7061)
    T = rnd(rng, 600)
    p = 300                                                         # the seed, in template coordinates
    reads, meta = [], {}                                            # meta: read -> (window start, window end, reversed, tags)

    def total():
        return sum(len(r) for r in reads)

    def fill_to(res):
        reads.append(rnd(rng, 16 + (res - total() - 16) % 16))      # (16 .. 31 bases: not a "short predecessor")
        assert total() % 16 == res

    def window(a0, a1, rev, *tags):
        w = T[a0:a1]
        reads.append(rc(w) if rev else w)
        meta[len(reads) - 1] = (a0, a1, rev, tags)
        return len(reads) - 1

    tests = [window(100, 485, False, "first_read")]
    fill_to(1)
    tests.append(window(110, 492, True, "start1"))
    fill_to(15)
    tests.append(window(105, 476, False, "start15"))
    reads.append(rnd(rng, 7))
    tests.append(window(120, 480, False, "short_pred"))
    reads.append(rnd(rng, 15))
    tests.append(window(115, 470, True, "short_pred"))
    big = {False: window(40, 560, False), True: window(40, 560, True)}
    w = rnd(rng, 150)
    reads.append(w + rc(w))
    pal = len(reads) - 1
    fill_to(0)
    tests.append(window(125, 471, False, "start0"))
    fill_to((total_mod - 377) % 16)
    tests.append(window(108, 485, True, "last_read"))
    assert total() % 16 == total_mod
    cs.seqs = reads

    def pos(r):
        a0, a1, rev, _ = meta[r]
        return a1 - p - k if rev else p - a0
    for r in tests:
        rev = meta[r][2]
        for strand in STRANDS:
            b = big[rev ^ (strand == "c")]
            cs.seeds.append((r, b, pos(r), pos(b)))
            cs.labels.append(dict(event="place", which="H", read=r, strand=strand, tags=meta[r][3]))
            cs.seeds.append((b, r, pos(b), pos(r)))
            cs.labels.append(dict(event="place", which="V", read=r, strand=strand, tags=meta[r][3]))
    r = tests[3]
    cs.seeds.append((r, r, pos(r), pos(r)))
    cs.labels.append(dict(event="same_read", strand="n", read=r))
    cs.seeds.append((pal, pal, 60, 300 - 60 - k))
    cs.labels.append(dict(event="same_read", strand="c", read=pal))
    return cs


# ---- parameters -----------------------------------------------------------------------------------------------------------------
KS = (11, 17, 32)
XS = (1, 7, 60, 100, 127)
NOISE = ("identical", 0.03, 0.15, "identical", 0.03, "unrelated", "mismatch")


@functools.lru_cache(None)
def _mixed_reads():
    rng = np.random.default_rng(7071)
    seqs, plan = [], []
    for n in range(300):
        L = int(200 + 1200 * np.sqrt(rng.random()))                                     # 200 .. 1,400, the long ones more often
        tpl = rng.integers(0, 4, L).astype(np.uint8)
        s0 = int(rng.integers(0, L - 32 + 1)) if n % 5 else (0 if n % 2 else L - 32)   # the seed's 32 bases stay: every k fits
        cut_l = int(rng.integers(0, s0 + 1)) if n % 3 else 0
        cut_r = int(rng.integers(s0 + 32, L + 1)) if n % 3 == 1 else L
        col = tpl[cut_l:cut_r].copy()
        sj = s0 - cut_l
        noise = NOISE[n % len(NOISE)]
        if noise == "unrelated":
            mut = np.ones(len(col), bool)
            new = rng.integers(0, 4, len(col)).astype(np.uint8)
        elif noise == "mismatch":
            mut = np.ones(len(col), bool)
            new = (col + 1 + rng.integers(0, 3, len(col))) % 4
        else:
            mut = rng.random(len(col)) < (0.0 if noise == "identical" else noise)
            new = (col + rng.integers(1, 4, len(col))) % 4
        mut[sj:sj + 32] = False
        col = np.where(mut, new, col).astype(np.uint8)
        seqs += [synth.BASES[tpl].tobytes(), synth.BASES[col].tobytes()]
        plan.append((s0, sj, (n // len(NOISE)) % 2 == 1, noise))
    return seqs, plan


@functools.lru_cache(None)
def mixed_set(k: int, X: int) -> CaseSet:
    """300 pairs of 200 .. 1,400 bases: identical, 3 %, 15 %, unrelated and never-matching flanks, unequal lengths, both strands,
    seeds anywhere including the very ends; under every k and X"""
    seqs, plan = _mixed_reads()
    cs = CaseSet("mixed-k%d-x%d" % (k, X), k, X)
    for n, (s0, sj, rev, noise) in enumerate(plan):
        row, col = seqs[2 * n], seqs[2 * n + 1]
        if rev:
            col, sj = rc(col), len(col) - k - sj
        cs.add_pair(row, col, s0, sj, event="mixed", noise=noise, strand="c" if rev else "n")
    return cs


# ---- survivors and batches ------------------------------------------------------------------------------------------------------
SURVIVOR_SEEDS = 2350
SURVIVOR_JUNK = 100


@functools.lru_cache(None)
def survivor_set() -> CaseSet:
    """six copies of one 2,300-base read (a few substitutions each, three stored as reverse complements) and 2,350 seeds within 40
    bases of the middle: 4,700 extensions of more than 4 x 512 steps each, so more than 4,096 survive four launches; and 100 pairs
    of unrelated short reads, spread among them, that end in the first launch"""
    k = 17
    cs = CaseSet("survivor", k, 15)
    rng = np.random.default_rng(7081)
    L, mid = 2300, 1150
    tpl = rng.integers(0, 4, L).astype(np.uint8)
    revs = []
    for r in range(6):
        c = tpl.copy()
        mut = rng.random(L) < 0.003
        mut[mid - 80:mid + 80] = False
        c[mut] = (c[mut] + rng.integers(1, 4, int(mut.sum()))) % 4
        s = synth.BASES[c].tobytes()
        revs.append(r % 2 == 1)
        cs.seqs.append(rc(s) if revs[-1] else s)
    todo = [(a, b, d) for d in range(-40, 41) for a in range(6) for b in range(6) if a != b][:SURVIVOR_SEEDS]
    every = len(todo) // SURVIVOR_JUNK
    for n, (a, b, d) in enumerate(todo):
        p = mid + d
        cs.seeds.append((a, b, L - p - k if revs[a] else p, L - p - k if revs[b] else p))
        cs.labels.append(dict(event="survivor", strand="c" if revs[a] != revs[b] else "n"))
        if n % every == 0 and n // every < SURVIVOR_JUNK:
            seed = rnd(rng, k)
            x, y = rnd(rng, 60), rnd(rng, 60)
            cs.add_pair(x[:40] + seed + x[40:], y[:45] + seed + y[45:], 40, 45, event="junk")
    return cs


def tiny_set() -> CaseSet:
    """three pairs: what a second call on an engine that has just run the survivor set gets"""
    cs = CaseSet("tiny", 17, 7)
    rng = np.random.default_rng(7091)
    t = rnd(rng, 400)
    cs.add_pair(t[:300], t[50:], 100, 50, event="tiny")
    cs.add_pair(rc(t[:300]), t[50:], 300 - 100 - 17, 50, event="tiny")
    cs.add_pair(t[:200], rnd(rng, 90) + t[100:117] + rnd(rng, 90), 100, 90, event="tiny")
    return cs


def boundary_sets():
    return [drop_set(), end_set(), tail_drop_set(), kept_set(100), kept_set(127), early_set()]


def small_sets():
    """every set but the parameter sweep and the survivor set"""
    return boundary_sets() + [flank_set()] + [place_set(m) for m in (0, 1, 15)]


def slice_default(header_text: str) -> int:
    """the default of BELLA_XDROP_SLICE as xdrop_packed.hpp states it"""
    import re
    m = re.search(r"#ifndef BELLA_XDROP_SLICE\s*\n\s*#define BELLA_XDROP_SLICE (\d+)", header_text)
    return int(m.group(1))
