"""numpy / plain-Python statement of tip clipping, unitig compaction and unitig sequences and of the unitig
consensus (section 14), on the reduced string graph of graph_mirror (section 11's notation: vertex 2 r + o, twin(v -> w) = (w ^ 1 -> v ^ 1), in-degree(v) = out-degree(v ^ 1)).
Written straight from the definition; everything is an integer, so the device result must EQUAL it."""
from __future__ import annotations

import numpy as np

from . import graph_mirror as G

LINK_DT = np.dtype([("a", "<u4"), ("b", "<u4"), ("ovl", "<u4"), ("rec", "<u4"), ("flags", "<u4"), ("edge", "<u4")])
assert LINK_DT.itemsize == 24
LINK_A_MINUS, LINK_B_MINUS = 1, 2
CLEAN_DEFAULTS = dict(max_tip_reads=4, tip_rounds=3)
MAX_TIP_ROUNDS = 16
END, OUT, IN, LONG = "END", "OUT", "IN", "LONG"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s: bytes) -> bytes:
    return bytes(s).translate(_COMP)[::-1]


def tip_walk(off, dst, v, max_tip_reads):
    """the walk from start vertex v on one snapshot: -> (chain, reason)"""
    deg = lambda x: off[x + 1] - off[x]
    chain, cur = [v], v
    while True:
        if deg(cur) == 0:
            return chain, END
        if deg(cur) > 1:
            return chain, OUT
        w = dst[off[cur]]
        if deg(w ^ 1) != 1:
            return chain, IN
        if len(chain) == max_tip_reads:
            return chain, LONG
        chain.append(w)
        cur = w


def clean(offsets, edges, contained, **kw):
    """bella_hip_graph_clean: -> dict(offsets, edges, removed (uint8), rounds = [(tips, reads)] of every round that ran)"""
    p = dict(CLEAN_DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError("unknown clean parameter %r" % k)
        p[k] = int(v)
    if not 0 <= p["tip_rounds"] <= MAX_TIP_ROUNDS:
        raise ValueError("tip_rounds")
    nv = len(offsets) - 1
    removed = np.zeros(nv // 2, bool)
    e = np.array(edges, G.EDGE_DT)
    off = np.asarray(offsets).astype(np.int64)
    rounds = []
    for _ in range(p["tip_rounds"] if p["max_tip_reads"] else 0):
        o, dst = off.tolist(), e["dst"].tolist()
        hit = np.zeros(nv // 2, bool)
        tips = 0
        for v in range(nv):
            if o[(v ^ 1) + 1] - o[v ^ 1] == 0 and o[v + 1] - o[v] >= 1:
                chain, why = tip_walk(o, dst, v, p["max_tip_reads"])
                if why in (IN, OUT):
                    tips += 1
                    hit[[x >> 1 for x in chain]] = True
        rounds.append((tips, int(hit.sum())))
        if not hit.any():
            break
        assert not (hit & removed).any()
        removed |= hit
        e = e[~(hit[e["src"] >> 1] | hit[e["dst"] >> 1])]
        cnt = np.zeros(nv + 1, np.int64)
        np.add.at(cnt, e["src"].astype(np.int64) + 1, 1)
        off = np.cumsum(cnt)
    return dict(offsets=off.astype(np.uint64), edges=e, removed=removed.astype(np.uint8), rounds=rounds)


def n50(lens):
    """the length of the unitig at which the sum of the lengths, largest first, reaches half of the total (0 without unitigs)"""
    tot, acc = int(sum(int(x) for x in lens)), 0
    for x in sorted((int(x) for x in lens), reverse=True):
        acc += x
        if 2 * acc >= tot:
            return x
    return 0


def unitigs(offsets, edges, contained, removed, lens):
    """bella_hip_graph_unitigs without the bases: -> dict(voff uint64[n + 1], verts uint32, pos uint64, nbases uint32, len uint64[n],
    circular uint8[n], links of LINK_DT, largest, n50, total_bases)"""
    off = [int(x) for x in offsets]
    nv = len(off) - 1
    lens = [int(x) for x in lens]
    dead = np.asarray(contained, bool) | (np.asarray(removed, bool) if removed is not None else False)
    dst, eln = edges["dst"].tolist(), edges["len"].tolist()
    deg = lambda x: off[x + 1] - off[x]
    succ, pred, out_len = [-1] * nv, [-1] * nv, [0] * nv
    merge = [False] * len(dst)
    for v in range(nv):
        if deg(v) == 1 and deg(dst[off[v]] ^ 1) == 1:
            w = dst[off[v]]
            assert pred[w] == -1
            succ[v], pred[w], out_len[v], merge[off[v]] = w, v, eln[off[v]], True
    for v in range(nv):                                               # mergeability is twin-symmetric
        assert succ[v] == -1 or succ[succ[v] ^ 1] == v ^ 1
    live = [not dead[v >> 1] for v in range(nv)]
    seen = [False] * nv
    paths = []                                                        # (vertices, circular), every path and its mirror
    for v in range(nv):
        if live[v] and pred[v] == -1:
            p = [v]
            while succ[p[-1]] != -1:
                p.append(succ[p[-1]])
            for x in p:
                assert not seen[x]
                seen[x] = True
            paths.append((p, False))
    for v in range(nv):
        if live[v] and not seen[v]:                                   # an all-mergeable cycle; v is its smallest vertex
            p = [v]
            while succ[p[-1]] != v:
                p.append(succ[p[-1]])
            for x in p:
                assert not seen[x] and x >= v
                seen[x] = True
            paths.append((p, True))
    assert all(seen[v] == live[v] for v in range(nv))
    emitted = [(p, c) for p, c in paths if (p[0] <= min(x ^ 1 for x in p) if c else p[0] <= p[-1] ^ 1)]
    emitted.sort(key=lambda pc: pc[0][0])
    voff, verts, pos, nb, ulen, circ = [0], [], [], [], [], []
    first, last = {}, {}                                              # vertex -> unitig, for the emitted paths' ends
    for u, (p, c) in enumerate(emitted):
        at = 0
        for i, v in enumerate(p):
            n = out_len[v] if i + 1 < len(p) else (eln[off[v]] if c else lens[v >> 1])
            verts.append(v); pos.append(at); nb.append(n)
            at += n
        voff.append(len(verts)); ulen.append(at); circ.append(1 if c else 0)
        if not c:
            first[p[0]], last[p[-1]] = u, u
    links = []
    for v in range(nv):
        for i in range(off[v], off[v + 1]):
            if merge[i]:
                continue
            w = dst[i]
            assert (v in last) != ((v ^ 1) in first) and (w in first) != ((w ^ 1) in last)      # a non-mergeable edge joins path ends
            a, fa = (last[v], 0) if v in last else (first[v ^ 1], LINK_A_MINUS)
            b, fb = (first[w], 0) if w in first else (last[w ^ 1], LINK_B_MINUS)
            links.append((a, b, int(edges["ovl"][i]), int(edges["rec"][i]), fa | fb, i))
    return dict(voff=np.array(voff, np.uint64), verts=np.array(verts, np.uint32), pos=np.array(pos, np.uint64), nbases=np.array(nb, np.uint32),
                len=np.array(ulen, np.uint64), circular=np.array(circ, np.uint8), links=np.array(links, LINK_DT) if links else np.zeros(0, LINK_DT),
                largest=max(ulen) if ulen else 0, n50=n50(ulen), total_bases=sum(ulen))


def unitig_bases(u, seqs):
    """-> (offsets uint64[n + 1], bases): vertex i contributes the first nbases[i] bases of its read in the vertex's orientation"""
    rc = {}
    out, offs = [], [0]
    voff = u["voff"].astype(np.int64).tolist()
    for k in range(len(u["len"])):
        for v, n in zip(u["verts"][voff[k]:voff[k + 1]].tolist(), u["nbases"][voff[k]:voff[k + 1]].tolist()):
            s = bytes(seqs[v >> 1])
            if v & 1:
                s = rc.setdefault(v >> 1, revcomp(s))
            out.append(s[:n])
        offs.append(offs[-1] + int(u["len"][k]))
    b = b"".join(out)
    assert len(b) == offs[-1]
    return np.array(offs, np.uint64), b


def check_invariants(u, offsets, edges, contained, removed, lens):
    """what holds on every input: every live read in exactly one emitted unitig, pos strictly increasing, len by the formula, links
    between path ends and in twin pairs"""
    dead = np.asarray(contained, bool) | np.asarray(removed, bool)
    reads = (u["verts"] >> 1).astype(np.int64)
    assert np.array_equal(np.sort(reads), np.flatnonzero(~dead))
    voff = u["voff"].astype(np.int64).tolist()
    at = {(int(s), int(d)): i for i, (s, d) in enumerate(zip(edges["src"].tolist(), edges["dst"].tolist()))}
    for k in range(len(u["len"])):
        v, p, n = (u[f][voff[k]:voff[k + 1]].astype(np.int64) for f in ("verts", "pos", "nbases"))
        assert len(v) >= 1 and p[0] == 0 and np.all(np.diff(p) > 0) and np.array_equal(np.cumsum(n) - n, p)
        el = [int(edges["len"][at[(int(a), int(b))]]) for a, b in zip(v[:-1], v[1:])]
        if u["circular"][k]:
            el.append(int(edges["len"][at[(int(v[-1]), int(v[0]))]]))
            assert int(u["len"][k]) == sum(el) and v[0] == v.min()
        else:
            assert int(u["len"][k]) == sum(el) + int(lens[v[-1] >> 1])
    assert np.all(np.diff(u["verts"][u["voff"][:-1].astype(np.int64)].astype(np.int64)) > 0)       # ordered by first vertex
    L = u["links"]
    assert np.all(np.diff(L["edge"].astype(np.int64)) > 0)
    end_a = {}
    for k in range(len(u["len"])):
        if not u["circular"][k]:
            f, l = int(u["verts"][voff[k]]), int(u["verts"][voff[k + 1] - 1])
            end_a[(k, 0)], end_a[(k, 1)] = l, f ^ 1                  # the vertex a link leaves from: + the last vertex, - the first one's twin
    have = set()
    for a, b, ovl, rec, fl, ei in L.tolist():
        s, d = int(edges["src"][ei]), int(edges["dst"][ei])
        assert end_a[(a, fl & 1)] == s and end_a[(b, 1 - (fl >> 1 & 1))] == d ^ 1
        assert ovl == int(edges["ovl"][ei]) and rec == int(edges["rec"][ei])
        have.add((a, fl & 1, b, fl >> 1 & 1, rec))
    assert len(have) == len(L) and all((b, 1 - fb, a, 1 - fa, rec) in have for a, fa, b, fb, rec in have)      # twin pairs


def unitig_names(u):
    return ["utg%06d%s" % (k + 1, "c" if c else "l") for k, c in enumerate(u["circular"].tolist())]


def unitig_gfa_text(names, u, offsets=None, bases=None) -> bytes:
    """GFA 1 as bella_hip_write_unitig_gfa writes it; bases = None: '*' for every sequence"""
    nm = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    un = [n.encode() for n in unitig_names(u)]
    voff = u["voff"].astype(np.int64).tolist()
    out = [b"H\tVN:Z:1.0\n"]
    for k, name in enumerate(un):
        seq = b"*" if bases is None else bytes(bases[int(offsets[k]):int(offsets[k + 1])])
        out.append(b"S\t%s\t%s\tLN:i:%d\tRC:i:%d\n" % (name, seq, int(u["len"][k]), voff[k + 1] - voff[k]))
        for i in range(voff[k], voff[k + 1]):
            v = int(u["verts"][i])
            out.append(b"a\t%s\t%d\t%s\t%s\t%d\n" % (name, int(u["pos"][i]), nm[v >> 1], b"-" if v & 1 else b"+", int(u["nbases"][i])))
    for a, b, ovl, rec, fl, _ in u["links"].tolist():
        out.append(b"L\t%s\t%s\t%s\t%s\t%dM\trc:i:%d\n" % (un[a], b"-" if fl & LINK_A_MINUS else b"+", un[b], b"-" if fl & LINK_B_MINUS else b"+", ovl, rec))
    return b"".join(out)


def fasta_text(u, offsets, bases) -> bytes:
    return b"".join(b">%s\n%s\n" % (n.encode(), bytes(bases[int(offsets[k]):int(offsets[k + 1])])) for k, n in enumerate(unitig_names(u)))


# ---- unitig consensus ----------------------------------------------------------------------------------------------
POLISH_DT = np.dtype([("len_before", "<u8"), ("len_after", "<u8"), ("substituted", "<u8"), ("deleted", "<u8"), ("inserted", "<u8"), ("covered", "<u8"),
                      ("depth_sum", "<u8")])
_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
_ASCII = np.frombuffer(b"ACGT", np.uint8)
BRANCHES = ("depth0", "below", "at", "del_major", "del_tie", "ins_major", "ins_tie", "sub", "tie_own", "tie_other")


def decisions(read: bytes, rows, min_depth: int = 3):
    """Section 10's rule at every position p of one read, from ITS rows of the table ((len, 9)): dict of per-position arrays --
    ins (bool: the junction before p emits), ins_base, keep (bool: the position emits), base (codes), sub / cov (bool), depth -- and
    `branch`, which branches of the rule the rows took (BRANCHES -> count)."""
    own = _CODE[np.frombuffer(bytes(read), np.uint8)].astype(np.int64)
    n = len(own)
    T = np.asarray(rows, np.int64).reshape(n, 9)
    p = np.arange(n)
    depth = T[:, 0:4].sum(1) + T[:, 4]
    prev = np.concatenate([[0], depth[:-1]])
    c = np.minimum(prev, depth)
    I = T[:, 5:9].sum(1)
    junction = (p >= 1) & (c >= min_depth)
    ins = junction & (2 * I > c + 1)
    ins_base = T[:, 5:9].argmax(1) if n else np.zeros(0, np.int64)               # the first maximum: ties go to the smallest code
    cov = depth >= min_depth
    dele = cov & (2 * T[:, 4] > depth + 1)
    w = T[:, 0:4].copy()
    w[p, own] += 1
    mx = w.max(1) if n else np.zeros(0, np.int64)
    own_max = w[p, own] == mx
    call = np.where(own_max, own, w.argmax(1) if n else own)
    base = np.where(cov, call, own)
    voted = cov & ~dele
    nmax = (w == mx[:, None]).sum(1) if n else np.zeros(0, np.int64)
    branch = dict(depth0=int((depth == 0).sum()), below=int(((depth > 0) & ~cov).sum()), at=int((depth == min_depth).sum()), del_major=int(dele.sum()),
                  del_tie=int((cov & (2 * T[:, 4] == depth + 1)).sum()), ins_major=int(ins.sum()), ins_tie=int((junction & (2 * I == c + 1)).sum()),
                  sub=int((voted & (base != own)).sum()), tie_own=int((voted & (nmax > 1) & own_max).sum()), tie_other=int((voted & (nmax > 1) & ~own_max).sum()))
    return dict(ins=ins, ins_base=ins_base, keep=~dele, base=base, sub=voted & (base != own), cov=cov, depth=depth, dele=dele, branch=branch)


def polished(u, seqs, table, min_depth: int = 3):
    """bella_hip_graph_polish_unitigs: -> dict(offsets uint64[n + 1], bases, pos uint64 / nbases uint32 per vertex in polished coordinates,
    len uint64[n], stats of POLISH_DT per unitig).  table: (total bases, 9), the rows of all reads in read order.  Vertex i = 2 r + o
    with n = nbases[i] contributes E(0) .. E(n - 1) for o = 0 and rc(E(L - 1)) .. rc(E(L - n)) for o = 1, E(p) = the decision string
    at position p of read r: the junction's base if it fires, then the position's base unless it is deleted."""
    lens = np.array([len(x) for x in seqs], np.int64)
    roff = np.concatenate([[0], np.cumsum(lens)])
    T = np.asarray(table).reshape(-1, 9)
    assert len(T) == roff[-1] and min_depth >= 1
    dec = {}
    voff = u["voff"].astype(np.int64).tolist()
    out, offs, pos, nb, stats = [], [0], [], [], np.zeros(len(u["len"]), POLISH_DT)
    for k in range(len(u["len"])):
        at = 0
        for v, n in zip(u["verts"][voff[k]:voff[k + 1]].tolist(), u["nbases"][voff[k]:voff[k + 1]].tolist()):
            r, L = v >> 1, int(lens[v >> 1])
            if r not in dec:
                dec[r] = decisions(seqs[r], T[roff[r]:roff[r + 1]], min_depth)
            d = dec[r]
            idx = np.arange(L - 1, L - 1 - n, -1) if v & 1 else np.arange(n)
            slots, use = np.empty(2 * n, np.int64), np.empty(2 * n, bool)
            if v & 1:                                                 # rc of a decision string: the position's base first, then the junction's
                slots[0::2], slots[1::2] = 3 - d["base"][idx], 3 - d["ins_base"][idx]
                use[0::2], use[1::2] = d["keep"][idx], d["ins"][idx]
            else:
                slots[0::2], slots[1::2] = d["ins_base"][idx], d["base"][idx]
                use[0::2], use[1::2] = d["ins"][idx], d["keep"][idx]
            seg = _ASCII[slots[use]].tobytes()
            out.append(seg); pos.append(at); nb.append(len(seg))
            at += len(seg)
            st = stats[k]
            st["substituted"] += int(d["sub"][idx].sum()); st["deleted"] += int(d["dele"][idx].sum()); st["inserted"] += int(d["ins"][idx].sum())
            st["covered"] += int(d["cov"][idx].sum()); st["depth_sum"] += int(d["depth"][idx].sum())
        stats[k]["len_before"], stats[k]["len_after"] = int(u["len"][k]), at
        offs.append(offs[-1] + at)
    return dict(offsets=np.array(offs, np.uint64), bases=b"".join(out), pos=np.array(pos, np.uint64), nbases=np.array(nb, np.uint32),
                len=stats["len_after"].astype(np.uint64), stats=stats)


def polished_unitigs(u, p):
    """the unitig dict with its coordinates replaced by the polished ones: what unitig_gfa_text / fasta_text take with p's offsets and bases"""
    q = dict(u)
    q["pos"], q["nbases"], q["len"] = p["pos"], p["nbases"], p["len"]
    return q


def branch_counts(seqs, table, min_depth: int = 3):
    """BRANCHES -> how many positions of the read set took that branch of the rule"""
    lens = np.array([len(x) for x in seqs], np.int64)
    roff = np.concatenate([[0], np.cumsum(lens)])
    T = np.asarray(table).reshape(-1, 9)
    tot = dict.fromkeys(BRANCHES, 0)
    for r, s in enumerate(seqs):
        for k, x in decisions(s, T[roff[r]:roff[r + 1]], min_depth)["branch"].items():
            tot[k] += x
    return tot


def random_table(lens, seed, min_depth: int = 3):
    """A seeded (total bases, 9) uint32 table whose rows are drawn so that every branch of the rule occurs at `min_depth`: depth 0, depth
    below and exactly at min_depth, deletion majorities and exact ties (2 del == depth + 1), insertion majorities and ties, and small
    base counts, where two equal maxima with and without the read's own base among them are common."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(lens))
    T = np.zeros((n, 9), np.int64)
    kind = rng.integers(0, 10, n)
    one_hot = lambda m: np.eye(4, dtype=np.int64)[rng.integers(0, 4, m)]
    sel = lambda k: np.flatnonzero(kind == k)
    i = sel(1); T[i, 0:4] = one_hot(len(i)) * rng.integers(1, max(min_depth, 2), len(i))[:, None]             # below min_depth (min_depth 1: none)
    i = sel(2); T[i, 0:4] = one_hot(len(i)) * min_depth                                                        # exactly at it
    i = sel(3); T[i, 0:4] = rng.integers(0, 3, (len(i), 4)); T[i, 4] = T[i, 0:4].sum(1) + rng.integers(2, 9, len(i)) + min_depth      # deletion majority
    i = sel(4); T[i, 0:4] = rng.integers(0, 3, (len(i), 4)) + one_hot(len(i)) * min_depth; T[i, 4] = T[i, 0:4].sum(1) + 1             # 2 del == depth + 1
    i = sel(5); T[i, 0:4] = rng.integers(0, 4, (len(i), 4)); T[i, 4] = rng.integers(0, 2, len(i))                                     # small counts: ties
    i = sel(6); T[i, 0:4] = one_hot(len(i)) * rng.integers(min_depth, min_depth + 30, len(i))[:, None] + rng.integers(0, 3, (len(i), 4))   # one clear base
    i = np.flatnonzero(kind >= 7); T[i, 0:4] = rng.integers(0, 20, (len(i), 4)); T[i, 4] = rng.integers(0, 12, len(i))                # anything
    i = np.flatnonzero(rng.integers(0, 8, n) == 0); T[i, 0:5] *= 10                                                                  # some deep rows
    depth = T[:, 0:5].sum(1)
    c = np.minimum(np.concatenate([[0], depth[:-1]]), depth)                          # (a read's first row has no junction: its counters are just data)
    how = rng.integers(0, 4, n)                                                      # 0: none, 1: an exact tie where c is odd, 2: one over it, 3: anything
    I = np.select([how == 1, how == 2, how == 3], [(c + 1) // 2, (c + 1) // 2 + 1, rng.integers(0, 25, n)], 0)
    first = rng.integers(0, I + 1)                                                   # split I over two bases: equal ins maxima occur
    a, b = rng.integers(0, 4, n), rng.integers(0, 4, n)
    np.add.at(T, (np.arange(n), 5 + a), first)
    np.add.at(T, (np.arange(n), 5 + b), I - first)
    return T.astype(np.uint32)


def window_distance(window: bytes, template: bytes) -> int:
    """Levenshtein distance (unit costs) of `window` to the best PREFIX of `template`: the window is consumed whole, the template's end
    is free -- the minimum of the last row of pileup_mirror.edit_distance's table."""
    x, y = np.frombuffer(window, np.uint8), np.frombuffer(template, np.uint8)
    idx = np.arange(len(y) + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(1, len(x) + 1):
        cand = np.empty(len(y) + 1, np.int64)
        cand[0] = i
        np.minimum(prev[:-1] + (y != x[i - 1]), prev[1:] + 1, out=cand[1:])
        prev = np.minimum.accumulate(cand - idx) + idx
    return int(prev.min())


# ---- inputs of the tests ----------------------------------------------------------------------------------------------------------------
def tip_input():
    """40 reads of 10 kb every 2,000 bases on a line (random strands, seed 3) plus two reads at 41,000 and 42,500; the records between
    those two and main reads that start after 40,000 are deleted: -> (starts, lens, strands, recs)"""
    rng = np.random.default_rng(3)
    starts = np.concatenate([np.arange(40) * 2000, [41000, 42500]]).astype(np.int64)
    lens = np.full(42, 10000, np.int64)
    strands = rng.integers(0, 2, 42)
    recs = G.truth_records(starts, lens, strands)
    side = (recs["cid"] >= 40) | (recs["rid"] >= 40)
    main = np.where(recs["cid"] >= 40, recs["rid"], recs["cid"])
    drop = side & (recs["cid"] < 40) & (starts[main] > 40000)
    return starts, lens, strands, recs[~drop]


def two_round_input():
    """A main line of 30 reads 0 .. 29; read 30 overlaps the middle of the line from the side (30 -> 15, so 15 has two in-edges), and the
    reads 31 and 32 both overlap read 30 (31 -> 30, 32 -> 30, so 30 has two in-edges).  Round 1: 31 and 32 start walks that stop with IN at
    30; read 30 is no start (its in-degree is 2).  Round 2: 30 now has in-degree 0, its walk stops with IN at 15.  Found with the mirror;
    rounds = [(2, 2), (1, 1), (0, 0)] with the defaults.  -> (lens, recs), explicit records on reads of 10 kb"""
    L = 10000
    out = []
    rec = lambda a, b, shift: out.append((a, b, shift, L, 0, L - shift, 0, 0, (0, 0, 0)))          # a's suffix on b's prefix, b starts `shift` into a
    for i in range(29):
        rec(i, i + 1, 2000)
    rec(30, 15, 3000)
    rec(31, 30, 3000)
    rec(32, 30, 5000)
    return np.full(33, L, np.int64), np.array(out, G.OVL_DT)


def reads_from_genome(genome: bytes, starts, lens, strands):
    return [revcomp(genome[int(s):int(s) + int(n)]) if o else genome[int(s):int(s) + int(n)] for s, n, o in zip(starts, lens, strands)]


def random_genome(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, int(n))].tobytes()


def circle_input(nreads=60, read_len=10000, step=2000, seed=5, fan=4):
    """reads every `step` bases around a circular genome of nreads * step bases, mixed strands, explicit records to the next `fan` reads
    (the wrap-around ones included): -> (genome, seqs, strands, recs)"""
    glen = nreads * step
    genome = random_genome(glen, seed)
    strands = np.random.default_rng(seed + 1).integers(0, 2, nreads)
    dbl = genome + genome
    seqs = reads_from_genome(dbl, np.arange(nreads) * step, np.full(nreads, read_len), strands)
    out = []
    for a in range(nreads):
        for d in range(1, fan + 1):
            b = (a + d) % nreads
            sh = d * step                                             # b starts sh bases into a; they share [sh, read_len) of a, [0, read_len - sh) of b
            v, h = (a, b) if a < b else (b, a)
            ca, cb = (sh, read_len), (0, read_len - sh)               # on a, on b, in the genome's direction
            cv, ch = (ca, cb) if v == a else (cb, ca)
            if strands[v]:
                cv, ch = (read_len - cv[1], read_len - cv[0]), (read_len - ch[1], read_len - ch[0])
            out.append((v, h, cv[0], cv[1], ch[0], ch[1], read_len - sh, int(strands[v] ^ strands[h]), (0, 0, 0)))
    recs = np.array(out, G.OVL_DT)
    return genome, seqs, strands, recs[np.lexsort((recs["rid"], recs["cid"]))]


def short_segment_input(n=400, seed=17):
    """reads of 40 to 70 bases every 1 to 20 bases on a line, mixed strands, exact records: segments of 1 to 20 bases
    -> (starts, lens, strands, recs); built with min_overlap = 0, fuzz = 0 and no clipping it is one unitig"""
    rng = np.random.default_rng(seed)
    starts = np.cumsum(rng.integers(1, 21, n))
    lens = rng.integers(40, 71, n)
    strands = rng.integers(0, 2, n)
    return starts, lens, strands, G.truth_records(starts, lens, strands, min_overlap=1)


def polish_cases():
    """the layouts the polish tests share: -> [(name, seqs, recs, graph parameters, clean parameters)] -- the tip input (one unitig of
    88,000 bases; unclipped with max_tip_reads = 1 it is three unitigs), the circle, the two-round input and the short segments"""
    def cut(starts, lens, strands, seed):
        genome = random_genome(int((np.asarray(starts) + np.asarray(lens)).max()), seed)
        return reads_from_genome(genome, starts, lens, strands)
    out = []
    starts, lens, strands, recs = tip_input()
    seqs = cut(starts, lens, strands, 33)
    out.append(("tip", seqs, recs, {}, {}))
    out.append(("tip3", seqs, recs, {}, dict(max_tip_reads=1)))
    _, seqs, _, recs = circle_input()
    out.append(("circle", seqs, recs, {}, {}))
    lens, recs = two_round_input()
    out.append(("two_round", [random_genome(int(n), 40 + i) for i, n in enumerate(lens)], recs, {}, {}))
    starts, lens, strands, recs = short_segment_input()
    out.append(("short", cut(starts, lens, strands, 34), recs, dict(min_overlap=0, fuzz=0), dict(max_tip_reads=0)))
    return out


def case_unitigs(seqs, recs, graph, clean_params):
    """graph_mirror.build -> clean -> unitigs of one polish case: -> (graph, cleaned, unitigs)"""
    lens = np.array([len(x) for x in seqs], np.int64)
    m = G.build(recs, lens, **graph)
    c = clean(m["offsets"], m["edges"], m["contained"], **clean_params)
    return m, c, unitigs(c["offsets"], c["edges"], m["contained"], c["removed"], lens)
