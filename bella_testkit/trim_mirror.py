"""numpy statement of the coverage trimming: the clip of every read from the overlap records, the cut of the
records to the clips, and the graph, unitigs and polish of the clipped reads through the existing mirrors.  Written straight from the
definition; the device result must EQUAL it (everything is an integer)."""
from __future__ import annotations

import numpy as np

from . import graph_mirror as G
from . import unitig_mirror as U

CLIP_DT = np.dtype([("beg", "<u4"), ("end", "<u4"), ("nregions", "<u4"), ("max_depth", "<u4")])
assert CLIP_DT.itemsize == 16
DEFAULTS = dict(min_depth=3, end_clip=500, min_span=1000)
UNCOVERED = 2                  # the value of contained[] for an uncovered read (1: contained)


def _params(kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("unknown trim parameter %r" % k)
        p[k] = int(v)
    if p["min_depth"] < 1:
        raise ValueError("min_depth must be >= 1")
    return p


def own_intervals(recs, lens):
    """every record's interval on V and on H, both in the read's OWN coordinates: -> (b1, e1, b2, e2) int64"""
    lens = np.asarray(lens, np.int64)
    l2 = lens[recs["rid"].astype(np.int64)]
    s = recs["strand"] != 0
    b1, e1, b2, e2 = (recs[f].astype(np.int64) for f in ("begV", "endV", "begH", "endH"))
    return b1, e1, np.where(s, l2 - e2, b2), np.where(s, l2 - b2, e2)


def shrunk_intervals(recs, lens, **kw):
    """the intervals that enter the sweep: -> (read, s, t) int64, V's interval of every record first, then H's"""
    p = _params(kw)
    lens = np.asarray(lens, np.int64)
    cid, rid = recs["cid"].astype(np.int64), recs["rid"].astype(np.int64)
    b1, e1, b2, e2 = own_intervals(recs, lens)
    gives = (e1 - b1 >= p["min_span"]) & (e2 - b2 >= p["min_span"])
    read = np.concatenate([cid[gives], rid[gives]])
    b, e = np.concatenate([b1[gives], b2[gives]]), np.concatenate([e1[gives], e2[gives]])
    l = lens[read]
    s = np.where(b <= p["end_clip"], b, b + p["end_clip"])
    t = np.where(l - e <= p["end_clip"], e, e - p["end_clip"])
    keep = t > s
    return read[keep], s[keep], t[keep]


def regions(recs, lens, **kw):
    """every region of every read, ordered by (read, start): -> (read, start, end) int64, max_depth[nreads]"""
    p = _params(kw)
    nreads = len(lens)
    read, s, t = shrunk_intervals(recs, lens, **kw)
    key = np.concatenate([read << 32 | s, read << 32 | t])
    delta = np.concatenate([np.ones(len(s), np.int64), -np.ones(len(t), np.int64)])
    at, inv = np.unique(key, return_inverse=True)
    net = np.zeros(len(at), np.int64)
    np.add.at(net, inv, delta)
    depth = np.cumsum(net)                                            # after ALL events of a position; a read's events sum to zero
    rd, pos = at >> 32, at & 0xFFFFFFFF
    maxd = np.zeros(nreads, np.int64)
    np.maximum.at(maxd, rd, depth)
    cov = depth >= p["min_depth"]
    prev = np.concatenate([[False], cov[:-1]])
    first, after = np.flatnonzero(cov & ~prev), np.flatnonzero(~cov & prev)      # a read's last position has depth 0: a run never crosses reads
    assert len(first) == len(after) and np.all(rd[first] == rd[after])
    return rd[first], pos[first], pos[after], maxd


def clips(recs, lens, **kw):
    """bella_hip_graph_trim: -> CLIP_DT[nreads]"""
    p = _params(kw)
    nreads = len(lens)
    rd, a, b, maxd = regions(recs, lens, **kw)
    out = np.zeros(nreads, CLIP_DT)
    out["max_depth"] = maxd
    out["nregions"] = np.bincount(rd, minlength=nreads)
    order = np.lexsort((a, -(b - a), rd))                             # per read: the longest first, the leftmost on ties
    rd, a, b = rd[order], a[order], b[order]
    top = np.flatnonzero(np.concatenate([[True], rd[1:] != rd[:-1]])) if len(rd) else np.zeros(0, np.int64)
    ok = b[top] - a[top] >= p["min_span"]
    out["beg"][rd[top][ok]], out["end"][rd[top][ok]] = a[top][ok], b[top][ok]
    return out


def trim_stats(recs, lens, clip, **kw):
    """the integer fields of bella_trim_stats after the trim (records_outside: cut())"""
    lens = np.asarray(lens, np.int64)
    n = clip["end"].astype(np.int64) - clip["beg"]
    dead = n == 0
    return dict(intervals=len(shrunk_intervals(recs, lens, **kw)[0]), reads_clipped=int((~dead & ((clip["beg"] != 0) | (clip["end"] != lens))).sum()),
                reads_uncovered=int(dead.sum()), reads_multi=int((clip["nregions"] >= 2).sum()), bases_before=int(lens.sum()), bases_after=int(n.sum()))


def cut(recs, lens, clip):
    """the records cut to the clips: -> (records in clipped coordinates (an OUTSIDE record keeps its numbers), outside[n] bool, clipped
    lengths[nreads], dead[nreads] bool)"""
    lens = np.asarray(lens, np.int64)
    cid, rid = recs["cid"].astype(np.int64), recs["rid"].astype(np.int64)
    s = recs["strand"] != 0
    cb, ce = clip["beg"].astype(np.int64), clip["end"].astype(np.int64)
    dead = ce == cb
    b1, e1, b2, e2 = (recs[f].astype(np.int64) for f in ("begV", "endV", "begH", "endH"))
    l2 = lens[rid]
    cs1, ce1 = cb[cid], ce[cid]
    c2s, c2e = np.where(s, l2 - ce[rid], cb[rid]), np.where(s, l2 - cb[rid], ce[rid])
    db = np.maximum(0, np.maximum(cs1 - b1, c2s - b2))
    de = np.maximum(0, np.maximum(e1 - ce1, e2 - c2e))
    nb1, ne1, nb2, ne2 = b1 + db, e1 - de, b2 + db, e2 - de
    outside = dead[cid] | dead[rid] | (ne1 <= nb1) | (ne2 <= nb2)
    out = recs.copy()
    k = ~outside
    out["begV"][k], out["endV"][k], out["begH"][k], out["endH"][k] = (nb1 - cs1)[k], (ne1 - cs1)[k], (nb2 - c2s)[k], (ne2 - c2s)[k]
    return out, outside, ce - cb, dead


def build(recs, lens, clip, **graph_params):
    """bella_hip_graph_build while clips exist: graph_mirror's classes, lists and reduction on the cut records.  `rec` stays the index
    among ALL records; contained[] holds UNCOVERED for an uncovered read.  -> graph_mirror.build's dict plus outside, lens (clipped)"""
    p = G._params(graph_params)
    nreads = len(lens)
    crecs, outside, clens, dead = cut(recs, lens, clip)
    kept = np.flatnonzero(~outside)
    cls, cand, valid, contained = G.classify(crecs[kept], clens, **graph_params)
    cand["rec"][valid] = kept[cand["rec"][valid]]
    off, e = G.build_lists(nreads, cand, valid, contained)
    red = G.reduce(off, e, p["fuzz"])
    at = {(int(s), int(d)): i for i, (s, d) in enumerate(zip(e["src"].tolist(), e["dst"].tolist()))}
    twin = np.array([at[(d ^ 1, s ^ 1)] for s, d in zip(e["src"].tolist(), e["dst"].tolist())], np.int64)
    gone = red | red[twin] if len(e) else red
    fe = e[~gone]
    foff = np.zeros(2 * nreads + 1, np.int64)
    np.add.at(foff, fe["src"].astype(np.int64) + 1, 1)
    deg = np.diff(off)
    stats = dict(records=len(recs), n_short=int((cls == G.SHORT).sum()), n_internal=int((cls == G.INTERNAL).sum()), contained_reads=int(contained.sum()),
                 edges_all=int(valid.sum()), edges_kept=len(e), edges_reduced=int(red.sum()), edges_final=len(fe), max_degree=int(deg.max()) if len(deg) else 0)
    assert not np.any(contained & dead)
    flags = contained.astype(np.uint8) + np.where(dead, UNCOVERED, 0).astype(np.uint8)
    return dict(offsets=np.cumsum(foff).astype(np.uint64), edges=fe, contained=flags, stats=stats, cls=cls, before=(off, e), outside=outside, lens=clens,
                records_outside=int(outside.sum()))


def clip_seqs(seqs, clip):
    """seq[beg:end] of every read"""
    return [bytes(s)[int(c["beg"]):int(c["end"])] for s, c in zip(seqs, clip)]


def trimmed_fasta_text(names, seqs, clip) -> bytes:
    """the FASTA of the clipped reads in input order, without the uncovered ones"""
    nm = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    return b"".join(b">%s\n%s\n" % (n, s) for n, s, c in zip(nm, clip_seqs(seqs, clip), clip) if c["end"] > c["beg"])


def polished(u, seqs, table, clip, min_depth: int = 3):
    """bella_hip_graph_polish_unitigs while clips exist: unitig_mirror.decisions on the FULL rows of every read (the junction rule and the
    table are in original coordinates), indexed through the clip: vertex 2 r + o with n bases takes the decisions of positions beg .. beg +
    n - 1 (o = 0) or end - 1 .. end - n (o = 1).  -> unitig_mirror.polished's dict"""
    lens = np.array([len(x) for x in seqs], np.int64)
    roff = np.concatenate([[0], np.cumsum(lens)])
    T = np.asarray(table).reshape(-1, 9)
    assert len(T) == roff[-1] and min_depth >= 1
    dec = {}
    voff = u["voff"].astype(np.int64).tolist()
    out, offs, pos, nb, stats = [], [0], [], [], np.zeros(len(u["len"]), U.POLISH_DT)
    for k in range(len(u["len"])):
        at = 0
        for v, n in zip(u["verts"][voff[k]:voff[k + 1]].tolist(), u["nbases"][voff[k]:voff[k + 1]].tolist()):
            r = v >> 1
            cs, ce = int(clip["beg"][r]), int(clip["end"][r])
            if r not in dec:
                dec[r] = U.decisions(seqs[r], T[roff[r]:roff[r + 1]], min_depth)
            d = dec[r]
            idx = np.arange(ce - 1, ce - 1 - n, -1) if v & 1 else np.arange(cs, cs + n)
            slots, use = np.empty(2 * n, np.int64), np.empty(2 * n, bool)
            if v & 1:
                slots[0::2], slots[1::2] = 3 - d["base"][idx], 3 - d["ins_base"][idx]
                use[0::2], use[1::2] = d["keep"][idx], d["ins"][idx]
            else:
                slots[0::2], slots[1::2] = d["ins_base"][idx], d["base"][idx]
                use[0::2], use[1::2] = d["ins"][idx], d["keep"][idx]
            seg = U._ASCII[slots[use]].tobytes()
            out.append(seg); pos.append(at); nb.append(len(seg))
            at += len(seg)
            st = stats[k]
            st["substituted"] += int(d["sub"][idx].sum()); st["deleted"] += int(d["dele"][idx].sum()); st["inserted"] += int(d["ins"][idx].sum())
            st["covered"] += int(d["cov"][idx].sum()); st["depth_sum"] += int(d["depth"][idx].sum())
        stats[k]["len_before"], stats[k]["len_after"] = int(u["len"][k]), at
        offs.append(offs[-1] + at)
    return dict(offsets=np.array(offs, np.uint64), bases=b"".join(out), pos=np.array(pos, np.uint64), nbases=np.array(nb, np.uint32),
                len=stats["len_after"].astype(np.uint64), stats=stats)


# ---- input makers -------------------------------------------------------------------------------------------------------------------------
def _record(v, iv, h, ih, lh, strand, score):
    """a record from the two reads' intervals in their OWN coordinates (v < h)"""
    hb, he = (lh - ih[1], lh - ih[0]) if strand else ih
    return (v, h, iv[0], iv[1], hb, he, score, strand, (0, 0, 0))


def junk_ends(starts, lens, strands, recs, frac=0.3, lo=1200, hi=3000, seed=11):
    """`frac` of the reads get lo .. hi junk bases in front, `frac` behind (independently, in the read's own direction); no record
    reaches into the junk.  -> (lens with the junk, the records in the new coordinates, head[nreads], tail[nreads]): the exact clip of read r
    is (head[r], head[r] + the old length)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    head = np.where(rng.random(n) < frac, rng.integers(lo, hi + 1, n), 0)
    tail = np.where(rng.random(n) < frac, rng.integers(lo, hi + 1, n), 0)
    cid, rid = recs["cid"].astype(np.int64), recs["rid"].astype(np.int64)
    s = recs["strand"] != 0
    out = recs.copy()
    out["begV"] += head[cid].astype(np.int32); out["endV"] += head[cid].astype(np.int32)
    sh = np.where(s, tail[rid], head[rid]).astype(np.int32)           # H' begins with H's tail when H is reversed
    out["begH"] += sh; out["endH"] += sh
    return lens + head + tail, out, head, tail


def junk_seqs(seqs, head, tail, seed=12):
    """the reads with random bases as junk: head[r] in front of read r, tail[r] behind"""
    return [U.random_genome(int(h), seed + 2 * i) + bytes(s) + U.random_genome(int(t), seed + 2 * i + 1) for i, (s, h, t) in enumerate(zip(seqs, head, tail))]


def chimeras(starts, lens, strands, recs, count=40, min_gap=30000, seed=13):
    """`count` new reads, each read a followed by read b (own directions) of two reads whose starts lie more than min_gap apart; every
    record of a and of b is repeated for the chimera, which takes the next read id and is therefore always H.  -> (lens, records, ids of
    the chimeras, (a, b) per chimera)"""
    rng = np.random.default_rng(seed)
    starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
    n = len(lens)
    b1, e1, b2, e2 = own_intervals(recs, lens)
    by_read = {}
    for i, (c, r) in enumerate(zip(recs["cid"].tolist(), recs["rid"].tolist())):
        by_read.setdefault(c, []).append(i)
        by_read.setdefault(r, []).append(i)
    new_lens, out, pairs = lens.tolist(), [], []
    while len(pairs) < count:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if abs(int(starts[a]) - int(starts[b])) <= min_gap:
            continue
        cid_new = n + len(pairs)
        L = int(lens[a] + lens[b])
        for part, shift in ((a, 0), (b, int(lens[a]))):
            for i in by_read.get(part, []):
                c, r, st = int(recs["cid"][i]), int(recs["rid"][i]), int(recs["strand"][i])
                other, io, ip = (r, (int(b2[i]), int(e2[i])), (int(b1[i]), int(e1[i]))) if c == part else (c, (int(b1[i]), int(e1[i])), (int(b2[i]), int(e2[i])))
                out.append(_record(other, io, cid_new, (ip[0] + shift, ip[1] + shift), L, st, int(recs["score"][i])))
        new_lens.append(L)
        pairs.append((a, b))
    allrecs = np.concatenate([recs, np.array(out, G.OVL_DT)]) if out else recs.copy()
    allrecs = allrecs[np.lexsort((allrecs["rid"], allrecs["cid"]))]
    return np.array(new_lens, np.int64), allrecs, np.arange(n, n + count), pairs


def hand_cases():
    """small inputs with their clips worked out by hand: -> [(name, lens, recs, trim parameters, expected (beg, end, nregions, max_depth) per read)]
    Every record lies on V = read 0 with its own H, so read 0 is the one under test; the H reads see one interval each (uncovered at
    min_depth >= 2)."""
    def recs_on0(ivs, l0, lh=20000, strand=0):
        out = []
        for k, (b, e) in enumerate(ivs):
            out.append(_record(0, (b, e), k + 1, (0, e - b), lh, strand, e - b))
        return np.array(out, G.OVL_DT), np.array([l0] + [lh] * len(ivs), np.int64)
    cases = []
    p = dict(min_depth=3, end_clip=0, min_span=1000)
    H = lambda n, d=1: [(0, 0, 0, d)] * n                             # the H reads: one interval each, never min_depth
    # depth exactly min_depth on [3000, 6000)
    r, l = recs_on0([(1000, 6000), (2000, 7000), (3000, 8000)], 10000)
    cases.append(("exact_depth", l, r, p, [(3000, 6000, 1, 3)] + H(3)))
    # two regions that abut at 5000: [2000, 5000) and [5000, 8000) from disjoint triples are one region
    r, l = recs_on0([(2000, 5000)] * 3 + [(5000, 8000)] * 3, 10000)
    cases.append(("abut", l, r, p, [(2000, 8000, 1, 3)] + H(6)))
    # a tie: [1000, 3000) and [5000, 7000): the leftmost
    r, l = recs_on0([(1000, 3000)] * 3 + [(5000, 7000)] * 3, 10000)
    cases.append(("tie_leftmost", l, r, p, [(1000, 3000, 2, 3)] + H(6)))
    # end_clip 500: intervals at the read's ends keep them, inner ends move: [0, 4000) x3 -> [0, 3500); [6000, 10000) x3 -> [6500, 10000); a tie
    q = dict(min_depth=3, end_clip=500, min_span=1000)
    r, l = recs_on0([(0, 4000)] * 3 + [(6000, 10000)] * 3, 10000)
    cases.append(("ends_kept", l, r, q, [(0, 3500, 2, 3)] + H(6)))
    # within end_clip of the ends counts as reaching them: [400, 9700) stays
    r, l = recs_on0([(400, 9700)] * 3, 10000)
    cases.append(("near_ends", l, r, q, [(400, 9700, 1, 3)] + H(3)))
    # end_clip 0 on the same records as ends_kept
    r, l = recs_on0([(0, 4000)] * 3 + [(6000, 10000)] * 3, 10000)
    cases.append(("end_clip_0", l, r, p, [(0, 4000, 2, 3)] + H(6)))
    # a read with no records (read 4), and the longest region shorter than min_span
    r, l = recs_on0([(1000, 5000), (2000, 6000), (4100, 9000)], 10000)
    l = np.concatenate([l, [7000]])
    cases.append(("short_and_none", l, r, p, [(0, 0, 1, 3)] + H(3) + [(0, 0, 0, 0)]))
    # strand 1: H's interval is mirrored into its own coordinates: H' [0, 3000) of 20,000 is H [17000, 20000)
    r, l = recs_on0([(1000, 4000)] * 3, 10000, strand=1)
    r["begH"], r["endH"] = 0, 3000
    cases.append(("strand1", l, r, dict(min_depth=1, end_clip=0, min_span=1000), [(1000, 4000, 1, 3)] + [(17000, 20000, 1, 1)] * 3))
    for name, l, r, _, want in cases:
        G.check_records(r, l)
        assert len(want) == len(l), name
    return cases
