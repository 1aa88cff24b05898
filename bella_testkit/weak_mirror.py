"""numpy / plain-Python statement of weak-overlap removal on the string graph, in the notation of sections 11 to 13
(vertex 2 r + o, twin(v -> w) = (w ^ 1 -> v ^ 1), a vertex's out-edges in list order, that is by (len, dst)).

Definition, integers only, on one snapshot of the current graph:
  best(v) = the largest ovl among v's out-edges.  They share the source read's length and ovl = that length - len, so best(v) is the ovl of
            the first edge of v's list (asserted here; the kernel relies on it).
  e = v -> w is WEAK iff 1000 ovl(e) < ratio_permille best(v).  With ratio_permille <= 1000 the best edge of a vertex is never weak, so a
            vertex with one out-edge loses nothing by its own rule.
  An edge leaves when it OR ITS TWIN is weak: the graph stays twin-symmetric.  No read is removed; a read left without edges becomes a
  one-vertex unitig.  The result is the CSR in the old order with the deleted edges compacted out.
Written straight from the definition, so the device result must EQUAL it.  The inputs of the tests are here too, and the schedule of the
command line (cut with a rising ratio, tips and bubbles again after every cut that took an edge)."""
from __future__ import annotations

import numpy as np

from . import bubble_mirror as B
from . import graph_mirror as G
from . import unitig_mirror as U

WEAK_DEFAULTS = dict(ratio_permille=500)
SCHEDULE_DEFAULTS = dict(weak_min=500, weak_max=700, weak_steps=2)
MAX_WEAK_STEPS = 16


def cut(offsets, edges, ratio_permille=500):
    """bella_hip_graph_cut_weak: -> dict(offsets, edges, forks, weak, edges_removed).  ratio_permille 0 is off: nothing is looked at, the
    figures are zero."""
    r = int(ratio_permille)
    if not 0 <= r <= 1000:
        raise ValueError("ratio_permille")
    e = np.array(edges, G.EDGE_DT)
    off = np.asarray(offsets).astype(np.int64)
    nv = len(off) - 1
    if r == 0 or len(e) == 0:
        return dict(offsets=off.astype(np.uint64), edges=e, forks=0, weak=0, edges_removed=0)
    src, dst, ovl = e["src"].astype(np.int64), e["dst"].astype(np.int64), e["ovl"].astype(np.int64)
    best = ovl[off[src]]
    largest = np.zeros(nv, np.int64)
    np.maximum.at(largest, src, ovl)
    assert np.array_equal(best, largest[src]), "the first edge of a list carries the vertex's largest overlap"
    weak = 1000 * ovl < r * best
    at = {sd: i for i, sd in enumerate(zip(src.tolist(), dst.tolist()))}
    twin = np.array([at[(d ^ 1, s ^ 1)] for s, d in zip(src.tolist(), dst.tolist())], np.int64)
    gone = weak | weak[twin]
    e = e[~gone]
    return dict(offsets=B._csr(nv, e).astype(np.uint64), edges=e, forks=int((np.diff(off) >= 2).sum()), weak=int(weak.sum()), edges_removed=int(gone.sum()))


def ratios(weak_min=500, weak_max=700, weak_steps=2):
    """the ratios of the command line's schedule: weak_steps + 1 of them, rising from weak_min to weak_max (integer division)"""
    lo, hi, n = int(weak_min), int(weak_max), int(weak_steps)
    if not (0 < lo <= hi <= 1000 and 0 <= n <= MAX_WEAK_STEPS):
        raise ValueError("0 < weak_min <= weak_max <= 1000 and 0 <= weak_steps <= %d" % MAX_WEAK_STEPS)
    return [lo + (hi - lo) * i // n if n else lo for i in range(n + 1)]


def schedule(offsets, edges, contained, removed, lens, weak_min=500, weak_max=700, weak_steps=2, clean_params=None, bubble_params=None):
    """What bella-hip --cut-weak does after its clean and its optional pop, on their graph and removed flags: for every ratio of ratios()
    cut; if the cut took an edge, U.clean with clean_params and, when bubble_params is not None, B.pop with them (miniasm's order: del_short,
    cut_tip, pop_bubble).  -> dict(offsets, edges, removed (uint8), steps): a step is dict(ratio_permille, forks, weak, edges_removed,
    reads_clipped, bubbles_popped, offsets, edges, removed, unitigs = how many unitigs the graph after the step has)."""
    off, e = np.asarray(offsets).astype(np.uint64), np.array(edges, G.EDGE_DT)
    nr = (len(off) - 1) // 2
    rem = np.zeros(nr, np.uint8) if removed is None else np.asarray(removed, np.uint8).copy()
    steps = []
    for r in ratios(weak_min, weak_max, weak_steps):
        c = cut(off, e, r)
        off, e = c["offsets"], c["edges"]
        step = dict(ratio_permille=r, forks=c["forks"], weak=c["weak"], edges_removed=c["edges_removed"], reads_clipped=0, bubbles_popped=0)
        if c["edges_removed"]:
            k = U.clean(off, e, contained, **(clean_params or {}))
            assert not (k["removed"] & rem).any()
            off, e, rem = k["offsets"], k["edges"], rem | k["removed"]
            step["reads_clipped"] = int(k["removed"].sum())
            if bubble_params is not None:
                p = B.pop(off, e, contained, rem, **bubble_params)
                off, e, rem = p["offsets"], p["edges"], p["removed"]
                step["bubbles_popped"] = sum(x[2] for x in p["rounds"])
        step.update(offsets=off, edges=e, removed=rem.copy(), unitigs=len(U.unitigs(off, e, contained, rem, lens)["len"]))
        steps.append(step)
    return dict(offsets=off, edges=e, removed=rem, steps=steps)


# ---- inputs of the tests: explicit overlap records on dummy reads of 10 kb (bubble_mirror.Layout) ----------------------------------
def two_lines_layout(spur=False):
    """two lines of 30 reads, 2,000 bases apart, and two false links between them: a10 -> b20 at shift 7,000 and b8 -> a22 at shift
    6,500 -- what a repeat with a copy in either line leaves.  spur: two more reads, a10 -> x0 -> x1 with good overlaps and a third false
    link x1 -> b25 at shift 7,000: closed at both ends, so no tip, until the cut takes x1 -> b25 and leaves x0, x1 hanging off a10"""
    y = B.Layout()
    a, b = ["a%d" % i for i in range(30)], ["b%d" % i for i in range(30)]
    y.read(*a)
    y.read(*b)
    y.path(a)
    y.path(b)
    y.link("a10", "b20", 7000)
    y.link("b8", "a22", 6500)
    if spur:
        y.link("a10", "x0", 2500)
        y.link("x0", "x1", 2000)
        y.link("x1", "b25", 7000)
    return y


def one_sided_layout():
    """a line of 30 reads and a read x whose only edge is x -> m15 at shift 7,000: not weak at x (one out-edge), weak at m15 ^ 1"""
    y = B.Layout()
    main = ["m%d" % i for i in range(30)]
    y.read(*main)
    y.path(main)
    y.link("x", "m15", 7000)
    return y


def fork_layout(shift_a, shift_b):
    """p0 -> p1 -> s, then s -> a0 -> a1 -> a2 at shift_a and s -> b0 -> b1 -> b2 at shift_b (the arms go on at 2,000)"""
    y = B.Layout()
    y.path(["p0", "p1", "s"])
    y.link("s", "a0", shift_a)
    y.path(["a0", "a1", "a2"])
    y.link("s", "b0", shift_b)
    y.path(["b0", "b1", "b2"])
    return y


def named_inputs():
    """every input of the tests: name -> (lens, recs).  The layouts come in bubble_mirror's three variants."""
    out = {}

    def add(name, y):
        for var in B.VARIANTS:
            lens, recs, _, _ = y.build(var, seed=len(out))
            out["%s/%s" % (name, var)] = (lens, recs)
    add("two-lines", two_lines_layout())
    add("two-lines-spur", two_lines_layout(spur=True))
    add("one-sided", one_sided_layout())
    add("equal", fork_layout(2000, 2000))                             # both out-edges of s have ovl 8,000
    add("boundary", fork_layout(2000, 6000))                          # ovl 8,000 and 4,000
    add("line", B.line_input())
    for name, (lens, recs, _) in B.existing_inputs().items():          # tip input, circle, hub, truth chain
        out[name] = (lens, recs)
    out["empty/plain"] = (np.full(4, B.L, np.int64), np.zeros(0, G.OVL_DT))
    out["one-read/plain"] = (np.full(1, B.L, np.int64), np.zeros(0, G.OVL_DT))
    return out
