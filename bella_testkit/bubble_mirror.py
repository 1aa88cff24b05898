"""numpy / plain-Python statement of bubble popping on the reduced string graph, in the notation of sections 11
and 12 (vertex 2 r + o, twin(v -> w) = (w ^ 1 -> v ^ 1), in-degree(v) = out-degree(v ^ 1), a vertex's out-edges in list order).
Written straight from the definition; everything is an integer, so the device result must EQUAL it.  The inputs of the tests are here too."""
from __future__ import annotations

import numpy as np

from . import graph_mirror as G
from . import unitig_mirror as U

POP_DEFAULTS = dict(max_bubble_reads=64, max_bubble_dist=50000, bubble_rounds=3)
MAX_BUBBLE_READS = 255
MAX_BUBBLE_ROUNDS = 16
NO_CLAIM = 0xFFFFFFFF


def _pop_params(kw):
    p = dict(POP_DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("unknown bubble parameter %r" % k)
        p[k] = int(v)
    if not 0 <= p["bubble_rounds"] <= MAX_BUBBLE_ROUNDS:
        raise ValueError("bubble_rounds")
    if not 0 <= p["max_bubble_reads"] <= MAX_BUBBLE_READS:
        raise ValueError("max_bubble_reads")
    return p


def detect(off, edges, s, p, order=None, why=None):
    """The Kahn traversal from source s on one snapshot.  off: offsets (ints), edges: (dst list, len list), p: dict with max_bubble_reads
    and max_bubble_dist.  order: None = the definition's order (last ready vertex first, edges in list order), else a numpy Generator that
    picks the ready vertex to pop and shuffles the order in which its edges are visited.  -> None on failure (the reason is appended to
    `why` when that is a list; it may depend on the order), else dict(t, visited = {vertex: dict(d, c, D, p)})."""
    dst, ln = edges
    deg = lambda x: off[x + 1] - off[x]
    fail = lambda reason: why.append(reason) if why is not None else None
    vis = {s: dict(r=0, d=0, c=0, D=0, p=s)}
    stack, pending = [s], 0
    while stack:
        v = stack.pop(int(order.integers(len(stack))) if order is not None else -1)
        if deg(v) == 0:
            return fail("tip")
        js = list(range(off[v], off[v + 1]))
        if order is not None:
            order.shuffle(js)
        rv = vis[v]
        for j in js:
            w, l = dst[j], ln[j]
            if w == s or (w ^ 1) in vis:
                return fail("cycle")
            if rv["d"] + l > p["max_bubble_dist"]:
                return fail("dist")
            if w not in vis:
                if len(vis) - 1 == p["max_bubble_reads"]:
                    return fail("reads")
                vis[w] = dict(r=deg(w ^ 1), d=rv["d"] + l, c=rv["c"] + 1, D=rv["D"] + l, p=v)
                pending += 1
            else:
                rw = vis[w]
                rw["d"] = min(rw["d"], rv["d"] + l)
                if (rv["c"] + 1, rv["D"] + l) > (rw["c"], rw["D"]) or ((rv["c"] + 1, rv["D"] + l) == (rw["c"], rw["D"]) and v < rw["p"]):
                    rw["c"], rw["D"], rw["p"] = rv["c"] + 1, rv["D"] + l, v
            vis[w]["r"] -= 1
            if vis[w]["r"] == 0:
                stack.append(w)
                pending -= 1
        if len(stack) == 1 and pending == 0:
            t = stack[0]
            assert deg(t ^ 1) >= 2 and s != t ^ 1 and all(x["r"] == 0 for x in vis.values())
            return dict(t=t, visited={x: {k: rec[k] for k in "dcDp"} for x, rec in vis.items()})
    return fail("open")


def kept_path(b, s):
    """t, p(t), p(p(t)), ... s"""
    k = [b["t"]]
    while k[-1] != s:
        k.append(b["visited"][k[-1]]["p"])
    return k


def _csr(nv, e):
    cnt = np.zeros(nv + 1, np.int64)
    np.add.at(cnt, e["src"].astype(np.int64) + 1, 1)
    return np.cumsum(cnt)


def pop_round(off, e, p):
    """one round on the snapshot (off, e): -> (hit bool[nreads], ekill bool[nedges], (sources, found, popped), bubbles found: {s: b})"""
    nv = len(off) - 1
    o = [int(x) for x in off]
    lists = (e["dst"].tolist(), e["len"].tolist())
    dst = lists[0]
    at = {(s_, d_): i for i, (s_, d_) in enumerate(zip(e["src"].tolist(), dst))}
    sources = [v for v in range(nv) if o[v + 1] - o[v] >= 2]
    all_found = {}
    for s in sources:
        b = detect(o, lists, s, p)
        if b is not None:
            all_found[s] = b
    for s, b in all_found.items():                                    # the mirror bubble is found from t ^ 1, with the same reads
        m = all_found.get(b["t"] ^ 1)
        if m is None:                                                 # (distances are measured from the other end there: only max_bubble_dist can differ)
            m = detect(o, lists, b["t"] ^ 1, dict(p, max_bubble_dist=1 << 62))
        assert m is not None and m["t"] == s ^ 1 and {x >> 1 for x in m["visited"]} == {x >> 1 for x in b["visited"]}
    found = {s: b for s, b in all_found.items() if s < (b["t"] ^ 1)}
    claim = np.full(nv // 2, NO_CLAIM, np.int64)
    interior = {s: [x for x in b["visited"] if x != s and x != b["t"]] for s, b in found.items()}
    for s, I in interior.items():
        for x in I:
            claim[x >> 1] = min(claim[x >> 1], s)
    hit = np.zeros(nv // 2, bool)
    ekill = np.zeros(len(e), bool)
    popped = 0
    for s, b in found.items():
        if any(claim[x >> 1] != s for x in interior[s]):
            continue
        popped += 1
        K = kept_path(b, s)
        kedges = set(zip(K[1:], K[:-1]))
        for x in interior[s]:
            if x not in K:
                hit[x >> 1] = True
        for v in b["visited"]:
            for j in range(o[v], o[v + 1]):
                w = dst[j]
                if w in b["visited"] and (v, w) not in kedges:
                    ekill[j] = True
                    ekill[at[(w ^ 1, v ^ 1)]] = True
    return hit, ekill, (len(sources), len(found), popped), all_found


def pop(offsets, edges, contained, removed, **kw):
    """bella_hip_graph_pop_bubbles: -> dict(offsets, edges, removed (uint8), rounds = [(sources, found, popped, reads, edges)] of every
    round that ran, sides = the canonical bubbles' sides seen: 0 when s is the forward vertex of its read, 1 when not)"""
    p = _pop_params(kw)
    nv = len(offsets) - 1
    rem = np.zeros(nv // 2, bool) if removed is None else np.asarray(removed, bool).copy()
    e = np.array(edges, G.EDGE_DT)
    off = np.asarray(offsets).astype(np.int64)
    rounds, sides = [], set()
    for _ in range(p["bubble_rounds"] if p["max_bubble_reads"] else 0):
        hit, ekill, (nsrc, nfound, npop), found = pop_round(off, e, p)
        sides |= {s & 1 for s, b in found.items() if s < (b["t"] ^ 1)}
        gone = hit[e["src"] >> 1] | hit[e["dst"] >> 1] | ekill if len(e) else ekill
        rounds.append((nsrc, nfound, npop, int(hit.sum()), int(gone.sum())))
        assert (nfound == 0) == (npop == 0)                              # the smallest source always wins: a round with a bubble makes progress
        if not npop:
            break
        assert not (hit & rem).any()
        rem |= hit
        e = e[~gone]
        off = _csr(nv, e)
    return dict(offsets=off.astype(np.uint64), edges=e, removed=rem.astype(np.uint8), rounds=rounds, sides=sides)


def check_graph(offsets, edges, removed):
    """after a pop: the graph is twin-symmetric and no edge touches a removed read"""
    have = set(zip(edges["src"].tolist(), edges["dst"].tolist()))
    assert len(have) == len(edges) and all((d ^ 1, s ^ 1) in have for s, d in have)
    rem = np.asarray(removed, bool)
    assert not (rem[edges["src"] >> 1] | rem[edges["dst"] >> 1]).any()
    assert np.array_equal(_csr(len(offsets) - 1, edges), np.asarray(offsets).astype(np.int64)) and np.all(np.diff(edges["src"].astype(np.int64)) >= 0)


def csr_from_edges(nreads, triples):
    """a hand-made graph: (v, w, len) triples, the twins added, lists ordered by (len, dst): -> (offsets, edges of EDGE_DT)"""
    both = {}
    for v, w, l in triples:
        both[(v, w)] = l
        both[(w ^ 1, v ^ 1)] = l
    e = np.zeros(len(both), G.EDGE_DT)
    for i, ((v, w), l) in enumerate(both.items()):
        e[i] = (v, w, l, 10000 - l, i, 0)
    e = e[np.lexsort((e["dst"], e["len"], e["src"]))]
    return _csr(2 * nreads, e).astype(np.uint64), e


# ---- inputs of the tests: explicit overlap records on dummy reads of 10 kb ------------------------------------------------------------
L = 10000


class Layout:
    """Reads named by the caller; link(a, b, shift): b starts `shift` bases into a (a's suffix on b's prefix), which gives the edge
    a+ -> b+ of length shift and its twin when both reads are on strand 0.  strands: 'random' (seeded) flips reads, `reverse` renumbers
    read i as n - 1 - i: the graph is the same up to the names of its vertices."""

    def __init__(self):
        self.names, self.links = [], []

    def read(self, *names):
        for n in names:
            assert n not in self.names
            self.names.append(n)

    def link(self, a, b, shift=2000):
        for n in (a, b):
            if n not in self.names:
                self.names.append(n)
        self.links.append((a, b, int(shift)))

    def path(self, names, shift=2000):
        for a, b in zip(names[:-1], names[1:]):
            self.link(a, b, shift)

    def build(self, variant="plain", seed=0, order=None):
        """-> (lens, recs, ids = {name: read id}, strands)"""
        n = len(self.names)
        names = list(order) + [x for x in self.names if x not in order] if order else list(self.names)
        ids = {nm: (n - 1 - i if variant == "reversed" else i) for i, nm in enumerate(names)}
        strands = np.random.default_rng(1000 + seed).integers(0, 2, n) if variant == "strands" else np.zeros(n, np.int64)
        out = []
        for a, b, sh in self.links:
            ia, ib = ids[a], ids[b]
            v, h = (ia, ib) if ia < ib else (ib, ia)
            ca, cb = (sh, L), (0, L - sh)                             # on a and on b, in the layout's direction
            cv, ch = (ca, cb) if v == ia else (cb, ca)
            if strands[v]:
                cv, ch = (L - cv[1], L - cv[0]), (L - ch[1], L - ch[0])
            out.append((v, h, cv[0], cv[1], ch[0], ch[1], L - sh, int(strands[v] ^ strands[h]), (0, 0, 0)))
        recs = np.array(out, G.OVL_DT) if out else np.zeros(0, G.OVL_DT)
        return np.full(n, L, np.int64), recs[np.lexsort((recs["rid"], recs["cid"]))], ids, strands


VARIANTS = ("plain", "strands", "reversed")


def simple_layout(kind):
    """a line of 30 reads m0 .. m29; an arm bypasses m14, m15.  kind 'count': the arm has 3 reads (the count decides: m14, m15 go);
    'length': 2 against 2, the arm's path is longer (D decides: m14, m15 go); 'pred': equal in both (the smaller predecessor decides)"""
    y = Layout()
    main = ["m%d" % i for i in range(30)]
    y.read(*main)
    y.path(main)
    if kind == "count":
        y.path(["m13", "x0", "x1", "x2", "m16"], 1500)
    elif kind == "length":
        y.link("m13", "x0", 2500); y.link("x0", "x1", 2000); y.link("x1", "m16", 2000)
    else:
        y.path(["m13", "x0", "x1", "m16"], 2000)
    return y


def direct_layout():
    """s -> a -> b -> t plus a direct s -> t of 3,000 bases that the reduction lets live: a's and b's lists do not name t and s's longest
    edge plus the fuzz is shorter than any two-edge way to t.  (With ONE read between s and t the build's reduction always takes the direct
    edge: step 3 looks at the first edge of every neighbour.  That graph is in literal_direct() for the mirror alone.)"""
    y = Layout()
    y.path(["p0", "p1", "s"])
    y.path(["s", "a", "b", "t"], 2500)
    y.link("s", "t", 3000)
    y.path(["t", "q0", "q1"])
    return y


def literal_direct():
    """s -> a -> t plus s -> t as a hand-made CSR on 5 reads (p, s, a, t, q): -> (offsets, edges)"""
    return csr_from_edges(5, [(0, 2, 2000), (2, 4, 2000), (4, 6, 2000), (2, 6, 3000), (6, 8, 2000)])


def nested_layout():
    y = Layout()
    y.path(["p0", "p1", "s"])
    y.link("s", "a"); y.link("a", "c", 1500); y.link("a", "d", 2500); y.link("c", "e", 2500); y.link("d", "e", 1500); y.link("e", "t")
    y.link("s", "b", 2500); y.link("b", "t", 2500)
    y.path(["t", "q0", "q1"])
    return y


NESTED_INNER_FIRST = ["a", "e", "c", "d", "p0", "p1", "s", "b", "t", "q0", "q1"]      # the inner source a is the smallest vertex
NESTED_OUTER_FIRST = ["s", "t", "p0", "p1", "a", "b", "c", "d", "e", "q0", "q1"]      # the outer source s is


def adjacent_layout():
    """two bubbles that share an end point: t of the first is s of the second"""
    y = Layout()
    y.path(["p0", "p1", "s"])
    y.path(["s", "a", "t"]); y.path(["s", "b", "t"], 2500)
    y.path(["t", "c", "u"]); y.path(["t", "d0", "d1", "u"], 1500)
    y.path(["u", "q0", "q1"])
    return y


def shared_sink_layout():
    """two forks that end in ONE vertex (in-degree 4): neither is closed, the other's in-edges come from outside"""
    y = Layout()
    y.path(["p0", "s1"]); y.path(["p1", "s2"])
    y.path(["s1", "a", "t"]); y.path(["s1", "b", "t"], 2500)
    y.path(["s2", "c", "t"], 1500); y.path(["s2", "d", "t"], 3000)
    y.path(["t", "q0", "q1"])
    return y


def refused_layout(kind):
    y = Layout()
    y.path(["p0", "p1", "s"])
    if kind == "tip":                                                 # b ends inside
        y.path(["s", "a", "t"]); y.link("s", "b", 2500)
    elif kind == "in":                                                # x -> a from outside
        y.path(["s", "a", "t"]); y.path(["s", "b", "t"], 2500); y.path(["x0", "x", "a"], 3000)
    elif kind == "out":                                               # a -> x to outside
        y.path(["s", "a", "t"]); y.path(["s", "b", "t"], 2500); y.path(["a", "x", "x0", "x1"], 3000)
    elif kind == "dist":                                              # refused with max_bubble_dist 5,000, popped with the default
        y.path(["s", "a", "t"], 3000); y.path(["s", "b0", "b1", "t"], 2500)
    elif kind == "reads3":                                            # visited - {s} = {a, b, t}: refused with max_bubble_reads 1 and 2
        y.path(["s", "a", "t"]); y.path(["s", "b", "t"], 2500)
    elif kind in ("reads255", "reads256"):                            # two arms, 255 or 256 reads with t
        na = 127 if kind == "reads255" else 128
        y.path(["s"] + ["a%d" % i for i in range(na)] + ["t"], 1500)
        y.path(["s"] + ["b%d" % i for i in range(127)] + ["t"], 1600)
    elif kind == "back":                                              # the arm a returns to s
        y.path(["s", "a", "t"]); y.path(["s", "b", "t"], 2500); y.link("a", "s", 3000)
    else:
        raise ValueError(kind)
    y.path(["t", "q0", "q1"])
    return y


def both_orientations():
    """a fork that would hold both orientations of a read: s -> a -> t, s -> b and one more record that lays a's suffix on the reverse
    complement of b (a+ -> b-, b+ -> a-).  -> (lens, recs)"""
    y = Layout()
    y.path(["p0", "p1", "s"])
    y.path(["s", "a", "t"]); y.link("s", "b", 2500)
    y.path(["t", "q0", "q1"])
    lens, recs, ids, _ = y.build()
    a, b = ids["a"], ids["b"]
    v, h = min(a, b), max(a, b)
    extra = np.array([(v, h, 3000, L, 0, 7000, 7000, 1, (0, 0, 0))], G.OVL_DT)
    recs = np.concatenate([recs, extra])
    return lens, recs[np.lexsort((recs["rid"], recs["cid"]))]


def chain_layout(seed, nbubbles=12, ends=2):
    """12 bubbles in a line, 2 or 3 arms each, 1 to 4 reads per arm, shifts of 1,500 to 4,000, `ends` reads before and after: -> Layout"""
    rng = np.random.default_rng(seed)
    y = Layout()
    y.path(["h%d" % i for i in range(ends)] + ["j0"])
    for k in range(nbubbles):
        for a in range(int(rng.integers(2, 4))):
            arm = ["b%d_%d_%d" % (k, a, i) for i in range(int(rng.integers(1, 5)))]
            names = ["j%d" % k] + arm + ["j%d" % (k + 1)]
            for x, z in zip(names[:-1], names[1:]):
                y.link(x, z, int(rng.integers(1500, 4001)))
    y.path(["j%d" % nbubbles] + ["z%d" % i for i in range(ends)])
    return y


def hub_input(nreads=3000, hub=700, band=8, Lh=20000):
    """a 700-way fork out of read 0 and an eight-wide band (the input of the unitig tests): -> (lens, recs)"""
    out = []
    for j in range(1, hub + 1):
        out.append((0, j, Lh // 2 + j, Lh, 0, Lh // 2 - j, 0, j & 1, (0, 0, 0)))
    for i in range(1, nreads - band):
        for d in range(1, band + 1):
            out.append((i, i + d, 1000 * d, Lh, 0, Lh - 1000 * d, 0, (i + d) % 3 == 0, (0, 0, 0)))
    out.append((nreads - 2, nreads - 1, 0, Lh, 0, Lh, 0, 0, (0, 0, 0)))
    return np.full(nreads, Lh, np.int64), np.array(out, G.OVL_DT)


def line_input(n=12):
    """edges, but no vertex with two out-edges"""
    y = Layout()
    y.path(["m%d" % i for i in range(n)])
    return y


def named_inputs():
    """every record-level input of the tests: name -> (lens, recs, pop parameters).  The layouts come in three variants each."""
    out = {}

    def add(name, y, params=None, **kw):
        for var in VARIANTS:
            lens, recs, _, _ = y.build(var, seed=len(out), **kw)
            out["%s/%s" % (name, var)] = (lens, recs, dict(params or {}))
    for kind in ("count", "length", "pred"):
        add("simple-" + kind, simple_layout(kind))
    add("direct", direct_layout())
    add("nested-inner", nested_layout(), order=NESTED_INNER_FIRST)
    add("nested-outer", nested_layout(), order=NESTED_OUTER_FIRST)
    add("adjacent", adjacent_layout())
    add("shared-sink", shared_sink_layout())
    for kind in ("tip", "in", "out", "back"):
        add("refused-" + kind, refused_layout(kind))
    add("refused-dist", refused_layout("dist"), dict(max_bubble_dist=5000))
    add("popped-dist", refused_layout("dist"))
    for mr in (1, 2):
        add("refused-reads%d" % mr, refused_layout("reads3"), dict(max_bubble_reads=mr))
    add("popped-reads3", refused_layout("reads3"), dict(max_bubble_reads=3))
    add("refused-reads255", refused_layout("reads256"), dict(max_bubble_reads=255, max_bubble_dist=1000000))
    add("popped-reads255", refused_layout("reads255"), dict(max_bubble_reads=255, max_bubble_dist=1000000))
    lens, recs = both_orientations()
    out["refused-both/plain"] = (lens, recs, {})
    for seed in range(20):
        y = chain_layout(seed)
        lens, recs, _, _ = y.build("strands", seed=seed)
        out["chain-%d/strands" % seed] = (lens, recs, {})
    add("line", line_input())
    out["empty/plain"] = (np.full(4, L, np.int64), np.zeros(0, G.OVL_DT), {})
    out["one-read/plain"] = (np.full(1, L, np.int64), np.zeros(0, G.OVL_DT), {})
    return out


def existing_inputs():
    """the inputs of the graph and unitig tests: name -> (lens, recs, pop parameters)"""
    out = {}
    starts, lens, strands, recs = U.tip_input()
    out["tip_input"] = (np.asarray(lens, np.int64), recs, {})
    genome, seqs, strands, recs = U.circle_input()
    out["circle_input"] = (np.array([len(s) for s in seqs], np.int64), recs, {})
    lens, recs = hub_input()
    out["hub"] = (lens, recs, {})
    starts, lens, strands, recs = G.truth_chain()
    out["truth_chain"] = (np.asarray(lens, np.int64), recs, {})
    return out


def dummy_seqs(lens, seed=77):
    rng = np.random.default_rng(seed)
    return [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(n))].tobytes() for n in lens]
