"""CPU tests of the statement of tip clipping and unitig compaction (bella_testkit/unitig_mirror.py): the mirror
alone, no device.  The device is held to this mirror in tests/test_unitig_gpu.py."""
import numpy as np
import pytest

from bella_testkit import graph_mirror as G
from bella_testkit import unitig_mirror as U


def _all(recs, lens, clean=None, **build):
    m = G.build(recs, lens, **build)
    c = U.clean(m["offsets"], m["edges"], m["contained"], **(clean or {}))
    u = U.unitigs(c["offsets"], c["edges"], m["contained"], c["removed"], lens)
    U.check_invariants(u, c["offsets"], c["edges"], m["contained"], c["removed"], lens)
    return m, c, u


def test_tip_input_clips_the_two_side_reads():
    starts, lens, strands, recs = U.tip_input()
    m, c, u = _all(recs, lens)
    assert len(m["edges"]) == 82 and np.diff(m["offsets"].astype(np.int64)).max() == 2 and not m["contained"].any()
    assert np.flatnonzero(c["removed"]).tolist() == [40, 41] and c["rounds"] == [(1, 2), (0, 0)]
    assert len(u["len"]) == 1 and not u["circular"][0] and len(u["links"]) == 0
    walk = u["verts"].tolist()
    if walk[0] >> 1 != 0:
        walk = [v ^ 1 for v in reversed(walk)]
    assert [v >> 1 for v in walk] == list(range(40)) and [v & 1 for v in walk] == strands[:40].tolist()
    assert int(u["len"][0]) == 39 * 2000 + 10000
    m1, c1, u1 = _all(recs, lens, clean=dict(max_tip_reads=1))           # the side chain has two reads: LONG
    assert not c1["removed"].any() and c1["rounds"] == [(0, 0)]
    assert len(u1["len"]) == 3 and len(u1["links"]) == 4
    m0, c0, u0 = _all(recs, lens, clean=dict(max_tip_reads=0))           # off: no round runs
    assert not c0["removed"].any() and c0["rounds"] == [] and c0["edges"].tobytes() == m["edges"].tobytes()


def test_truth_chain_is_one_unitig_in_line_order():
    starts, lens, strands, recs = G.truth_chain()
    m, c, u = _all(recs, lens)
    assert not c["removed"].any() and c["rounds"] == [(0, 0)] and len(m["edges"]) == 512
    order = [r for r in np.argsort(starts).tolist() if not m["contained"][r]]
    assert len(order) == 257 and len(u["len"]) == 1 and not u["circular"][0]
    walk = u["verts"].tolist()
    if walk[0] >> 1 != order[0]:
        walk = [v ^ 1 for v in reversed(walk)]
    assert [v >> 1 for v in walk] == order and [v & 1 for v in walk] == [int(strands[r]) for r in order]
    assert int(u["len"][0]) == int(starts[order[-1]] + lens[order[-1]] - starts[order[0]])


def test_a_second_round_clips_what_the_first_could_not():
    lens, recs = U.two_round_input()
    G.check_records(recs, lens)
    m, c, u = _all(recs, lens)
    assert c["rounds"] == [(2, 2), (1, 1), (0, 0)] and np.flatnonzero(c["removed"]).tolist() == [30, 31, 32]
    assert len(u["len"]) == 1 and sorted(v >> 1 for v in u["verts"].tolist()) == list(range(30))
    one = U.clean(m["offsets"], m["edges"], m["contained"], tip_rounds=1)
    assert one["rounds"] == [(2, 2)] and np.flatnonzero(one["removed"]).tolist() == [31, 32]


def test_circle_is_one_circular_unitig():
    genome, seqs, strands, recs = U.circle_input()
    lens = [len(s) for s in seqs]
    G.check_records(recs, lens)
    m, c, u = _all(recs, lens)
    assert u["circular"].tolist() == [1] and u["len"].tolist() == [120000] and len(u["verts"]) == 60 and len(u["links"]) == 0
    offs, b = U.unitig_bases(u, seqs)
    assert offs.tolist() == [0, 120000] and (b in genome + genome or U.revcomp(b) in genome + genome)


def test_bases_of_the_tip_input_are_the_main_line():
    starts, lens, strands, recs = U.tip_input()
    genome = U.random_genome(90000, 11)
    seqs = U.reads_from_genome(genome, starts, lens, strands)
    m, c, u = _all(recs, lens)
    offs, b = U.unitig_bases(u, seqs)
    assert b in (genome[:88000], U.revcomp(genome[:88000]))
    text = U.unitig_gfa_text(["r%d" % i for i in range(42)], u, offs, b)
    assert text.count(b"\nS\t") == 1 and text.count(b"\na\t") == 40 and b"\tLN:i:88000\tRC:i:40\n" in text
    assert U.fasta_text(u, offs, b) == b">utg000001l\n" + b + b"\n"
    assert U.n50([5, 3, 2]) == 5 and U.n50([3, 3, 2, 2]) == 3 and U.n50([]) == 0


@pytest.mark.parametrize("fuzz", [0, 1000])
def test_invariants_on_a_graph_with_forks(fuzz):
    """the band of tests/test_graph_gpu.py's hub input, smaller: forks, links, many unitigs"""
    L, n, band = 20000, 120, 4
    out = [(0, j, L // 2 + j, L, 0, L // 2 - j, 0, j & 1, (0, 0, 0)) for j in range(1, 31)]
    out += [(i, i + d, 1000 * d, L, 0, L - 1000 * d, 0, (i + d) % 3 == 0, (0, 0, 0)) for i in range(1, n - band) for d in range(1, band + 1)]
    recs, lens = np.array(out, G.OVL_DT), np.full(n, L, np.int64)
    for mt in (0, 1, 4):
        m, c, u = _all(recs, lens, clean=dict(max_tip_reads=mt), fuzz=fuzz)
        assert len(u["len"]) >= 1


def test_host_writers_equal_the_mirrors_text(tmp_path):
    """bella_hip_write_unitig_gfa and bella_hip_write_fasta (plain host code: no device) fed with the MIRROR's unitigs"""
    from bella_amd import api
    starts, lens, strands, recs = U.tip_input()
    genome = U.random_genome(90000, 11)
    seqs = U.reads_from_genome(genome, starts, lens, strands)
    names = ["r%d" % i for i in range(42)]
    for clean in ({}, dict(max_tip_reads=1)):                         # one unitig; three unitigs and four links
        m, c, u = _all(recs, lens, clean=clean)
        offs, b = U.unitig_bases(u, seqs)
        f = str(tmp_path / "u.gfa")
        api.write_unitig_gfa(f, names, u, offs, np.frombuffer(b, np.uint8))
        assert open(f, "rb").read() == U.unitig_gfa_text(names, u, offs, b)
        api.write_unitig_gfa(f, names, u)
        assert open(f, "rb").read() == U.unitig_gfa_text(names, u)
        f = str(tmp_path / "u.fa")
        api.write_fasta(f, api.unitig_names(u["circular"]), offs, np.frombuffer(b, np.uint8))
        assert open(f, "rb").read() == U.fasta_text(u, offs, b)
