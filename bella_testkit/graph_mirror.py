"""numpy / plain-Python statement of the string graph: overlap classes, containment, lists, Myers' transitive
reduction as miniasm states it, and the GFA text.  Written straight from the definition; the device result must EQUAL it (everything is
an integer)."""
from __future__ import annotations

import numpy as np

OVL_DT = np.dtype([("cid", "<u4"), ("rid", "<u4"), ("begV", "<i4"), ("endV", "<i4"), ("begH", "<i4"), ("endH", "<i4"), ("score", "<i4"),
                   ("strand", "u1"), ("pad", "u1", (3,))])
EDGE_DT = np.dtype([("src", "<u4"), ("dst", "<u4"), ("len", "<u4"), ("ovl", "<u4"), ("rec", "<u4"), ("flags", "<u4")])
assert OVL_DT.itemsize == 32 and EDGE_DT.itemsize == 24

DEFAULTS = dict(min_overlap=1000, max_overhang=1000, overhang_permille=800, fuzz=1000)
SHORT, INTERNAL, V_CONTAINED, H_CONTAINED, EDGE_V_FIRST, EDGE_H_FIRST = 1, 2, 3, 4, 5, 6
EDGE_TWIN = 1


def _params(kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("unknown graph parameter %r" % k)
        p[k] = int(v)
    return p


def check_records(recs, lens):
    """what bella_hip_graph_add_overlaps refuses"""
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    c, r = recs["cid"].astype(np.int64), recs["rid"].astype(np.int64)
    if np.any(c == r) or np.any(c >= n) or np.any(r >= n) or np.any(recs["strand"] > 1):
        raise ValueError("bad overlap record (ids / strand)")
    for b, e, l in ((recs["begV"], recs["endV"], lens[c]), (recs["begH"], recs["endH"], lens[r])):
        if np.any(b < 0) or np.any(b >= e) or np.any(e > l):
            raise ValueError("bad overlap record (coordinates)")


def classify(recs, lens, **kw):
    """-> (cls[n] of the six class codes, cand[2 n] of EDGE_DT: the record's edge and its twin at 2 i and 2 i + 1, valid[2 n],
    contained[nreads] bool)"""
    p = _params(kw)
    lens = np.asarray(lens, np.int64)
    n = len(recs)
    cid, rid, s = recs["cid"].astype(np.int64), recs["rid"].astype(np.int64), recs["strand"].astype(np.int64)
    b1, e1, b2, e2 = (recs[f].astype(np.int64) for f in ("begV", "endV", "begH", "endH"))
    l1, l2 = lens[cid], lens[rid]
    t1, t2 = l1 - e1, l2 - e2
    cls = np.zeros(n, np.uint8)
    short = (e1 - b1 < p["min_overlap"]) | (e2 - b2 < p["min_overlap"])
    overhang = np.minimum(b1, b2) + np.minimum(t1, t2)
    maplen = np.maximum(e1 - b1, e2 - b2)
    internal = ~short & ((overhang > p["max_overhang"]) | (1000 * overhang > p["overhang_permille"] * maplen))
    rest = ~short & ~internal
    vc = rest & (b1 <= b2) & (t1 <= t2)
    hc = rest & ~vc & (b1 >= b2) & (t1 >= t2)
    e5 = rest & ~vc & ~hc & (b1 > b2)
    e6 = rest & ~vc & ~hc & ~e5
    for code, m in ((SHORT, short), (INTERNAL, internal), (V_CONTAINED, vc), (H_CONTAINED, hc), (EDGE_V_FIRST, e5), (EDGE_H_FIRST, e6)):
        cls[m] = code
    contained = np.zeros(len(lens), bool)
    contained[cid[vc]] = True
    contained[rid[hc]] = True
    cand = np.zeros(2 * n, EDGE_DT)
    valid = np.zeros(2 * n, bool)
    v0, v1, hs, hn = 2 * cid, 2 * cid + 1, 2 * rid + s, 2 * rid + (s ^ 1)
    i5, i6 = np.flatnonzero(e5), np.flatnonzero(e6)
    for idx, first, twin in ((i5, (v0, hs, b1 - b2, l1), (hn, v1, t2 - t1, l2)), (i6, (hs, v0, b2 - b1, l2), (v1, hn, t1 - t2, l1))):
        for k, (src, dst, ln, lsrc) in enumerate((first, twin)):
            at = 2 * idx + k
            cand["src"][at], cand["dst"][at], cand["len"][at], cand["ovl"][at] = src[idx], dst[idx], ln[idx], lsrc[idx] - ln[idx]
            cand["rec"][at], cand["flags"][at] = idx, k * EDGE_TWIN
            valid[at] = True
    assert np.all(cand["len"][valid] > 0)
    return cls, cand, valid, contained


def build_lists(nreads, cand, valid, contained):
    """drops the edges with a contained end, orders every vertex's out-edges by (len, dst): -> (offsets[2 nreads + 1], edges)"""
    keep = valid & ~contained[cand["src"] >> 1] & ~contained[cand["dst"] >> 1]
    e = cand[keep]
    e = e[np.lexsort((e["dst"], e["len"], e["src"]))]
    key = e["src"].astype(np.int64) << 32 | e["dst"].astype(np.int64)
    if len(np.unique(key)) != len(key):
        raise ValueError("two records for one read pair")
    offsets = np.zeros(2 * nreads + 1, np.int64)
    np.add.at(offsets, e["src"].astype(np.int64) + 1, 1)
    return np.cumsum(offsets), e


def reduce(offsets, edges, fuzz):
    """-> reduced[nedges] bool: the edges step (4) marks"""
    off, dst, ln = [int(x) for x in offsets], edges["dst"].tolist(), edges["len"].tolist()
    reduced = np.zeros(len(edges), bool)
    INPLAY, ELIMINATED = 1, 2
    for v in range(len(off) - 1):
        a, b = off[v], off[v + 1]
        if a == b:
            continue
        mark = {dst[e]: INPLAY for e in range(a, b)}
        L = ln[b - 1] + fuzz
        for e in range(a, b):
            w = dst[e]
            if mark[w] != INPLAY:
                continue
            for f in range(off[w], off[w + 1]):
                if ln[e] + ln[f] > L:
                    break
                if mark.get(dst[f]) == INPLAY:
                    mark[dst[f]] = ELIMINATED
        for e in range(a, b):
            w = dst[e]
            for j, f in enumerate(range(off[w], off[w + 1])):
                if (j == 0 or ln[f] < fuzz) and mark.get(dst[f]) == INPLAY:
                    mark[dst[f]] = ELIMINATED
        for e in range(a, b):
            reduced[e] = mark[dst[e]] == ELIMINATED
    return reduced


def build(recs, lens, **kw):
    """the whole of bella_hip_graph_build: -> dict(offsets, edges, contained (uint8), stats, cls, before=(offsets, edges) before the reduction)"""
    p = _params(kw)
    nreads = len(lens)
    cls, cand, valid, contained = classify(recs, lens, **kw)
    off, e = build_lists(nreads, cand, valid, contained)
    red = reduce(off, e, p["fuzz"])
    at = {(int(s), int(d)): i for i, (s, d) in enumerate(zip(e["src"].tolist(), e["dst"].tolist()))}
    twin = np.array([at[(d ^ 1, s ^ 1)] for s, d in zip(e["src"].tolist(), e["dst"].tolist())], np.int64)
    gone = red | red[twin] if len(e) else red
    fe = e[~gone]
    foff = np.zeros(2 * nreads + 1, np.int64)
    np.add.at(foff, fe["src"].astype(np.int64) + 1, 1)
    deg = np.diff(off)
    stats = dict(records=len(recs), n_short=int((cls == SHORT).sum()), n_internal=int((cls == INTERNAL).sum()), contained_reads=int(contained.sum()),
                 edges_all=int(valid.sum()), edges_kept=len(e), edges_reduced=int(red.sum()), edges_final=len(fe), max_degree=int(deg.max()) if len(deg) else 0)
    return dict(offsets=np.cumsum(foff).astype(np.uint64), edges=fe, contained=contained.astype(np.uint8), stats=stats, cls=cls, before=(off, e))


def gfa_text(names, lens, seqs, offsets, edges, contained) -> bytes:
    """GFA 1 as bella_hip_write_gfa writes it; seqs = None: '*' for every sequence"""
    out = [b"H\tVN:Z:1.0\n"]
    nm = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    for r, n in enumerate(nm):
        if not contained[r]:
            out.append(b"S\t%s\t%s\tLN:i:%d\n" % (n, b"*" if seqs is None else bytes(seqs[r]), int(lens[r])))
    for e in edges.tolist():
        src, dst, ln, ovl, rec = e[:5]
        out.append(b"L\t%s\t%s\t%s\t%s\t%dM\tel:i:%d\trc:i:%d\n" % (nm[src >> 1], b"-" if src & 1 else b"+", nm[dst >> 1], b"-" if dst & 1 else b"+", ovl, ln, rec))
    return b"".join(out)


# ---- reads laid on a line: exact overlap records, and the walk along the reduced graph --------------------------------------------------
def truth_records(starts, lens, strands, min_overlap=1000):
    """Exact records of every read pair whose intervals [start, start + len) on a line share >= min_overlap bases.  strands[r] = 1: the
    read is the reverse complement of the line.  V = the smaller id, H = the larger (as the pipeline pairs them); coordinates on V and on
    H' = H oriented like V, so on a strand-1 V both are mirrored."""
    starts, lens, strands = (np.asarray(a, np.int64) for a in (starts, lens, strands))
    order = np.argsort(starts, kind="stable")
    ends = starts + lens
    out = []
    for ai, a in enumerate(order.tolist()):
        for b in order[ai + 1:].tolist():
            if starts[b] >= ends[a]:
                break
            lo, hi = max(starts[a], starts[b]), min(ends[a], ends[b])
            if hi - lo < min_overlap:
                continue
            v, h = (a, b) if a < b else (b, a)
            if strands[v] == 0:
                c = (lo - starts[v], hi - starts[v], lo - starts[h], hi - starts[h])
            else:
                c = (ends[v] - hi, ends[v] - lo, ends[h] - hi, ends[h] - lo)
            out.append((v, h, c[0], c[1], c[2], c[3], int(hi - lo), int(strands[v] ^ strands[h]), (0, 0, 0)))
    recs = np.array(out, OVL_DT) if out else np.zeros(0, OVL_DT)
    return recs[np.lexsort((recs["rid"], recs["cid"]))]


def truth_chain(nreads=500, seed=7, read_len=10000, spacing=300, min_overlap=1000):
    """~nreads reads with DISTINCT starts, mixed strands and jittered lengths on a line, from a fixed seed: (starts, lens, strands, recs)"""
    rng = np.random.default_rng(seed)
    starts = rng.permutation(np.cumsum(rng.integers(1, 2 * spacing, nreads)))
    lens = rng.integers(read_len - read_len // 10, read_len + read_len // 10, nreads)
    strands = rng.integers(0, 2, nreads)
    return starts, lens, strands, truth_records(starts, lens, strands, min_overlap)


def walk(offsets, edges, v):
    """follows the single out-edge from vertex v while there is exactly one; -> the vertices visited, v included"""
    off = [int(x) for x in offsets]
    seen, out = set(), []
    while v not in seen:
        seen.add(v)
        out.append(v)
        if off[v + 1] - off[v] != 1:
            break
        v = int(edges["dst"][off[v]])
    return out


def components(nreads, edges, contained):
    """weakly connected components among the non-contained reads"""
    parent = list(range(nreads))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for s, d in zip((edges["src"] >> 1).tolist(), (edges["dst"] >> 1).tolist()):
        parent[find(s)] = find(d)
    return len({find(r) for r in range(nreads) if not contained[r]})
