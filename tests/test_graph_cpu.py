"""CPU tests of the string graph: the numpy mirror (bella_testkit/graph_mirror.py) against hand-made cases and
against what follows from the definition on exact overlaps, and the library's GFA writer (plain host code) against the mirror's text."""
import numpy as np
import pytest

from bella_amd import _lib, api
from bella_testkit import graph_mirror as G


def _rec(cid, rid, bV, eV, bH, eH, strand=0, score=0):
    return (cid, rid, bV, eV, bH, eH, score, strand, (0, 0, 0))


def _csr(nv, triples):
    """lists from (src, dst, len): ordered by (len, dst) like build_lists"""
    e = np.zeros(len(triples), G.EDGE_DT)
    for i, (s, d, l) in enumerate(sorted(triples, key=lambda t: (t[0], t[2], t[1]))):
        e[i] = (s, d, l, 0, i, 0)
    off = np.zeros(nv + 1, np.int64)
    np.add.at(off, e["src"].astype(np.int64) + 1, 1)
    return np.cumsum(off), e


def test_dtypes_match_the_library():
    assert G.OVL_DT == _lib.OVL_DT and G.EDGE_DT == _lib.EDGE_DT
    assert G.DEFAULTS == api.Engine.GRAPH_DEFAULTS


@pytest.mark.parametrize("strand", [0, 1])
def test_the_six_classes(strand):
    """reads 0 (V, 10,000 bases) and 1 (H, 8,000 bases), one record per class; edge direction, orientation bits, len, ovl and the twin"""
    lens = np.array([10000, 8000])
    cases = {
        G.SHORT: _rec(0, 1, 9100, 10000, 0, 900, strand),
        G.INTERNAL: _rec(0, 1, 4000, 7000, 3000, 6000, strand),
        G.V_CONTAINED: _rec(0, 1, 0, 7000, 500, 7500, strand),             # (V's overhangs 0 / 3000 against 500 / 500: not contained ...)
        G.H_CONTAINED: _rec(0, 1, 1000, 9000, 0, 8000, strand),
        G.EDGE_V_FIRST: _rec(0, 1, 7000, 10000, 0, 3000, strand),
        G.EDGE_H_FIRST: _rec(0, 1, 0, 3000, 5000, 8000, strand),
    }
    cases[G.V_CONTAINED] = _rec(1, 0, 0, 8000, 1000, 9000, strand)          # V = read 1 lies inside H = read 0
    recs = np.array([cases[c] for c in sorted(cases)], G.OVL_DT)
    cls, cand, valid, contained = G.classify(recs, lens)
    assert cls.tolist() == sorted(cases)
    assert valid.tolist() == [False] * 8 + [True] * 4
    s = strand
    # class 5: V's suffix on H's prefix: (V,0) -> (H,s), len = b1 - b2; twin (H,s^1) -> (V,1), len = (l2 - e2) - (l1 - e1)
    assert cand[8].tolist() == (0, 2 + s, 7000, 3000, 4, 0) and cand[9].tolist() == (2 + (s ^ 1), 1, 5000, 3000, 4, G.EDGE_TWIN)
    # class 6: H's suffix on V's prefix: (H,s) -> (V,0), len = b2 - b1; twin (V,1) -> (H,s^1), len = (l1 - e1) - (l2 - e2)
    assert cand[10].tolist() == (2 + s, 0, 5000, 3000, 5, 0) and cand[11].tolist() == (1, 2 + (s ^ 1), 7000, 3000, 5, G.EDGE_TWIN)
    for a, b in ((8, 9), (10, 11)):
        assert cand[b]["src"] == cand[a]["dst"] ^ 1 and cand[b]["dst"] == cand[a]["src"] ^ 1
        assert cand[a]["ovl"] + cand[a]["len"] == lens[cand[a]["src"] >> 1] and cand[b]["ovl"] + cand[b]["len"] == lens[cand[b]["src"] >> 1]
    assert contained.tolist() == [False, True] or contained.tolist() == [True, True]
    # each containment record on its own
    assert G.classify(recs[2:3], lens)[3].tolist() == [False, True]         # V = read 1
    assert G.classify(recs[3:4], lens)[3].tolist() == [False, True]         # H = read 1
    # the permille test alone makes a record internal
    r = np.array([_rec(0, 1, 9000, 10000, 300, 1300, strand)], G.OVL_DT)    # overhang 300 on a 1000-base overlap
    assert G.classify(r, lens)[0].tolist() == [G.EDGE_V_FIRST] and G.classify(r, lens, overhang_permille=299)[0].tolist() == [G.INTERNAL]
    assert G.classify(r, lens, max_overhang=299)[0].tolist() == [G.INTERNAL] and G.classify(r, lens, min_overlap=1001)[0].tolist() == [G.SHORT]


def test_mutual_containment_equal_ends_is_v_contained():
    lens = np.array([5000, 5000])
    r = np.array([_rec(0, 1, 0, 5000, 0, 5000)], G.OVL_DT)
    cls, _, valid, contained = G.classify(r, lens)
    assert cls.tolist() == [G.V_CONTAINED] and not valid.any() and contained.tolist() == [True, False]


def test_bad_records_are_refused():
    lens = np.array([5000, 5000])
    for bad in (_rec(0, 0, 0, 10, 0, 10), _rec(0, 2, 0, 10, 0, 10), _rec(0, 1, 10, 10, 0, 10), _rec(0, 1, 0, 5001, 0, 10), _rec(0, 1, 0, 10, 0, 10, 2)):
        with pytest.raises(ValueError):
            G.check_records(np.array([bad], G.OVL_DT), lens)
    G.check_records(np.array([_rec(0, 1, 0, 5000, 0, 5000, 1)], G.OVL_DT), lens)


def _check_chain(offsets, edges, contained, starts, strands):
    deg = np.diff(offsets.astype(np.int64))
    assert deg.max() <= 1
    order = [r for r in np.argsort(starts).tolist() if not contained[r]]
    got = G.walk(offsets, edges, 2 * order[0] + int(strands[order[0]]))
    assert [v >> 1 for v in got] == order
    assert [v & 1 for v in got] == [int(strands[r]) for r in order]
    back = G.walk(offsets, edges, 2 * order[-1] + (int(strands[order[-1]]) ^ 1))
    assert [v >> 1 for v in back] == order[::-1]
    assert len(edges) == 2 * (len(order) - 1)


def test_truth_chain():
    """exact overlaps of ~500 reads on a line: lengths add up exactly, so the reduction leaves the chain of the non-contained reads, with
    fuzz 0 and with fuzz 1000"""
    starts, lens, strands, recs = G.truth_chain()
    assert len(np.unique(starts)) == len(starts) and 0 < strands.sum() < len(strands) and len(recs) > 5000
    G.check_records(recs, lens)
    res = {}
    for fuzz in (0, 1000):
        g = res[fuzz] = G.build(recs, lens, fuzz=fuzz)
        assert 0 < g["stats"]["contained_reads"] <= len(lens) - 50 and g["stats"]["n_internal"] == 0 and g["stats"]["n_short"] == 0
        assert g["stats"]["edges_final"] < g["stats"]["edges_kept"]
        _check_chain(g["offsets"], g["edges"], g["contained"], starts, strands)
    assert res[0]["edges"].tobytes() == res[1000]["edges"].tobytes() and np.array_equal(res[0]["offsets"], res[1000]["offsets"])


def test_myers_order_dependence():
    """a w eliminated earlier must not eliminate further; and an edge only step 3 removes"""
    v, w1, w2, x, y = 0, 1, 2, 3, 4
    base = [(v, w1, 1), (v, w2, 2), (v, x, 10), (w2, y, 1), (w2, x, 5)]
    off, e = _csr(5, base + [(w1, w2, 1)])
    red = G.reduce(off, e, 2)
    assert {(int(a["src"]), int(a["dst"])) for a in e[red]} == {(v, w2)}           # w2 was eliminated through w1: its list is not walked, x stays
    off, e = _csr(5, base)
    red = G.reduce(off, e, 2)
    assert {(int(a["src"]), int(a["dst"])) for a in e[red]} == {(v, x)}            # without w1 -> w2, w2 is INPLAY and reaches x (2 + 5 <= 10 + 2)
    # step 3 only: 10 + 1 > L = 10 + 0, but w -> x is the first edge of w's list
    off, e = _csr(3, [(0, 1, 10), (0, 2, 4), (1, 2, 1)])
    assert {(int(a["src"]), int(a["dst"])) for a in e[G.reduce(off, e, 0)]} == {(0, 2)}
    # ... and not when it is neither the first nor shorter than fuzz
    off, e = _csr(4, [(0, 1, 10), (0, 2, 4), (1, 3, 1), (1, 2, 3)])
    assert not G.reduce(off, e, 2).any()
    # step 3's other clause: a w that was eliminated still removes through its edges shorter than fuzz
    off, e = _csr(5, [(v, w1, 1), (v, w2, 2), (v, x, 10), (w1, w2, 1), (w2, y, 1), (w2, x, 2)])
    assert {(int(a["src"]), int(a["dst"])) for a in e[G.reduce(off, e, 3)]} == {(v, w2), (v, x)}
    assert {(int(a["src"]), int(a["dst"])) for a in e[G.reduce(off, e, 2)]} == {(v, w2)}


def test_duplicate_pair_raises():
    starts, lens, strands = [0, 2000, 4000], [5000, 5000, 5000], [0, 0, 0]
    recs = G.truth_records(starts, lens, strands)
    G.build(recs, lens)
    with pytest.raises(ValueError):
        G.build(np.concatenate([recs, recs[:1]]), lens)


FIVE = dict(starts=[0, 1000, 2000, 3000, 1200], lens=[3000, 3000, 3000, 3000, 500], strands=[0, 1, 0, 0, 0])


def _five():
    recs = G.truth_records(FIVE["starts"], FIVE["lens"], FIVE["strands"], 400)
    g = G.build(recs, FIVE["lens"], min_overlap=400)
    names = ["r%d" % i for i in range(5)]
    return recs, g, names


def test_gfa_text_of_five_reads():
    """four reads 1,000 bases apart (read 1 on the other strand) and a 500-base read inside reads 0 and 1: the chain 0 -> 1 -> 2 -> 3 and
    its twin, read 4 dropped"""
    recs, g, names = _five()
    assert g["contained"].tolist() == [0, 0, 0, 0, 1] and g["stats"]["edges_final"] == 6 and g["stats"]["edges_kept"] == 10
    txt = G.gfa_text(names, FIVE["lens"], None, g["offsets"], g["edges"], g["contained"])
    want = (b"H\tVN:Z:1.0\n"
            b"S\tr0\t*\tLN:i:3000\nS\tr1\t*\tLN:i:3000\nS\tr2\t*\tLN:i:3000\nS\tr3\t*\tLN:i:3000\n"
            b"L\tr0\t+\tr1\t-\t2000M\tel:i:1000\trc:i:0\n"
            b"L\tr1\t+\tr0\t-\t2000M\tel:i:1000\trc:i:0\n"
            b"L\tr1\t-\tr2\t+\t2000M\tel:i:1000\trc:i:3\n"
            b"L\tr2\t+\tr3\t+\t2000M\tel:i:1000\trc:i:6\n"
            b"L\tr2\t-\tr1\t+\t2000M\tel:i:1000\trc:i:3\n"
            b"L\tr3\t-\tr2\t-\t2000M\tel:i:1000\trc:i:6\n")
    assert txt == want, txt.decode()


def test_library_gfa_writer_equals_the_mirror(tmp_path):
    recs, g, names = _five()
    rng = np.random.default_rng(2)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist()) for n in FIVE["lens"]]
    f = str(tmp_path / "g.gfa")
    for sq in (None, seqs):
        api.write_gfa(f, names, FIVE["lens"], g["offsets"], g["edges"], g["contained"], seqs=sq)
        assert open(f, "rb").read() == G.gfa_text(names, FIVE["lens"], sq, g["offsets"], g["edges"], g["contained"])
    # an empty graph: header and every read
    e = G.build(np.zeros(0, G.OVL_DT), FIVE["lens"])
    api.write_gfa(f, names, FIVE["lens"], e["offsets"], e["edges"], e["contained"])
    assert open(f, "rb").read() == G.gfa_text(names, FIVE["lens"], None, e["offsets"], e["edges"], e["contained"]) and open(f, "rb").read().count(b"\nS\t") == 5
    with pytest.raises(api.BellaHipError):
        bad = g["edges"].copy()
        bad["dst"][0] = 99
        api.write_gfa(f, names, FIVE["lens"], g["offsets"], bad, g["contained"])
