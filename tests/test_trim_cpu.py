"""CPU tests of the coverage trimming: the mirror (bella_testkit/trim_mirror.py) against hand-worked cases and
against inputs whose right answer is known -- junk ends, chimeras --, the new structs against the header, the command line's argument
errors.  The device is held to this mirror in test_trim_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bella_amd import _lib, api
from bella_testkit import graph_mirror as G
from bella_testkit import trim_mirror as T
from bella_testkit import unitig_mirror as U
from conftest import ROOT


@pytest.mark.parametrize("case", T.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    """depth exactly at min_depth; abutting regions merge; a tie goes to the leftmost region; an interval at a read end keeps the end;
    end_clip = 0; a read with no records; the longest region shorter than min_span; strand-1 mirroring of H"""
    name, lens, recs, tp, want = case
    c = T.clips(recs, lens, **tp)
    assert [tuple(int(x) for x in row) for row in c.tolist()] == want
    st = T.trim_stats(recs, lens, c, **tp)
    assert st["reads_uncovered"] == sum(1 for w in want if w[0] == w[1]) and st["bases_after"] == sum(w[1] - w[0] for w in want)


def test_a_sweep_written_out_by_hand():
    """one read, events walked position by position in plain Python against the vectorised mirror"""
    rng = np.random.default_rng(3)
    for trial in range(50):
        n = int(rng.integers(1, 40))
        b = rng.integers(0, 20, n) * 250
        e = b + 1000 + rng.integers(0, 20, n) * 250
        recs = np.array([T._record(0, (int(x), int(y)), k + 1, (0, int(y - x)), 12000, int(k & 1), 0) for k, (x, y) in enumerate(zip(b, e))], G.OVL_DT)
        lens = np.full(n + 1, 12000, np.int64)
        p = dict(min_depth=int(rng.integers(1, 6)), end_clip=int(rng.choice([0, 100, 500])), min_span=int(rng.choice([1, 1000, 3000])))
        depth = np.zeros(12001, np.int64)
        for x, y in zip(b.tolist(), e.tolist()):
            if y - x < p["min_span"]:
                continue
            s = x if x <= p["end_clip"] else x + p["end_clip"]
            t = y if 12000 - y <= p["end_clip"] else y - p["end_clip"]
            if t > s:
                depth[s:t] += 1
        cov = np.concatenate([[False], depth >= p["min_depth"], [False]])
        starts, ends = np.flatnonzero(cov[1:] & ~cov[:-1]), np.flatnonzero(~cov[1:] & cov[:-1])
        best = (0, 0)
        for s, t in zip(starts.tolist(), ends.tolist()):
            if t - s > best[1] - best[0]:
                best = (s, t)
        if best[1] - best[0] < p["min_span"]:
            best = (0, 0)
        got = T.clips(recs, lens, **p)[0]
        assert (int(got["beg"]), int(got["end"]), int(got["nregions"]), int(got["max_depth"])) == (best[0], best[1], len(starts), int(depth.max())), (trial, p)


def test_cut():
    """the cut of the records: both sides move by the same amount; strand 1 mirrors H's clip into H' coordinates; a record that the cut
    empties, and a record with an uncovered read, are OUTSIDE"""
    lens = np.array([10000, 8000, 9000, 5000], np.int64)
    clip = np.zeros(4, T.CLIP_DT)
    clip["beg"], clip["end"] = [2000, 1000, 0, 0], [9000, 8000, 9000, 0]
    recs = np.array([
        (0, 1, 1500, 6000, 500, 5000, 0, 0, (0, 0, 0)),      # V clip 2000 moves b by 500, H clip 1000 by 500: db = 500; ends inside: de = 0
        (0, 1, 1500, 6000, 500, 5000, 0, 1, (0, 0, 0)),      # strand 1: H' clip = (8000 - 8000, 8000 - 1000) = (0, 7000): only V cuts, db = 500
        (0, 1, 8000, 10000, 0, 2000, 0, 0, (0, 0, 0)),       # V: e1 - ce1 = 1000; H: c2s - b2 = 1000: db = de = 1000 of 2000: emptied
        (0, 2, 0, 1000, 8000, 9000, 0, 0, (0, 0, 0)),        # V's clip begins at 2000: db = 2000 >= the record: emptied
        (0, 3, 3000, 6000, 0, 3000, 0, 0, (0, 0, 0)),        # read 3 is uncovered
        (0, 2, 2500, 9500, 1000, 8000, 0, 1, (0, 0, 0)),     # de = 500 from V; H' clip = (0, 9000): nothing from H
    ], G.OVL_DT)
    out, outside, clens, dead = T.cut(recs, lens, clip)
    assert outside.tolist() == [False, False, True, True, True, False] and clens.tolist() == [7000, 7000, 9000, 0] and dead.tolist() == [False, False, False, True]
    coords = lambda i: tuple(int(out[f][i]) for f in ("begV", "endV", "begH", "endH"))
    assert coords(0) == (2000 - 2000, 6000 - 2000, 1000 - 1000, 5000 - 1000)
    assert coords(1) == (0, 4000, 1000, 5000)
    assert coords(5) == (2500 - 2000, 9500 - 500 - 2000, 1000, 8000 - 500)
    m = T.build(recs, lens, clip, min_overlap=0)
    assert m["records_outside"] == 3 and m["contained"][3] == T.UNCOVERED and m["stats"]["records"] == 6
    assert set(m["edges"]["rec"].tolist()) <= {0, 1, 5}                 # rec: the index among ALL records


def test_junk_ends_break_the_graph_and_the_trim_mends_it():
    starts, lens, strands, recs = G.truth_chain(150)
    jl, jr, head, tail = T.junk_ends(starts, lens, strands, recs, 0.3, 1200, 3000)
    G.check_records(jr, jl)
    assert (head > 0).sum() > 20 and (tail > 0).sum() > 20
    plain = G.build(jr, jl)
    assert G.components(len(jl), plain["edges"], plain["contained"]) > 1 and plain["stats"]["n_internal"] > 0
    c = T.clips(jr, jl)
    m = T.build(jr, jl, c)
    assert G.components(len(jl), m["edges"], m["contained"] != 0) == 1 and m["stats"]["n_internal"] == 0
    print("TRIM junk_ends(truth_chain(150)): untrimmed %d components, %d internal; trimmed 1 component, 0 internal, %d records outside"
          % (G.components(len(jl), plain["edges"], plain["contained"]), plain["stats"]["n_internal"], m["records_outside"]))
    # end_clip = 0: exact, except on the reads at the genome's ends -- a read with fewer than min_depth reads starting before it (or ending
    # behind it) has an end that fewer than min_depth overlaps reach
    c0 = T.clips(jr, jl, end_clip=0)
    rank = np.argsort(np.argsort(starts))
    rank_end = np.argsort(np.argsort(starts + lens))
    inner = (rank >= 3) & (rank_end < len(lens) - 3)
    assert np.array_equal(c0["beg"][inner], head[inner]) and np.array_equal(c0["end"][inner], (head + lens)[inner])
    assert np.all(c0["beg"] >= head) and np.all(c0["end"] <= head + lens)          # never a junk base
    # the unitigs in clipped coordinates: one, and without the junk
    genome = U.random_genome(int((starts + lens).max()), 9)
    seqs = T.junk_seqs(U.reads_from_genome(genome, starts, lens, strands), head, tail)
    dead = (m["contained"] != 0).astype(np.uint8)
    cl = U.clean(m["offsets"], m["edges"], dead)
    u = U.unitigs(cl["offsets"], cl["edges"], dead, cl["removed"], m["lens"])
    _, b = U.unitig_bases(u, T.clip_seqs(seqs, c))
    assert len(u["len"]) == 1 and (b in genome or b in U.revcomp(genome))


def test_chimeras_split_with_the_shrink_and_only_with_it():
    starts, lens, strands, recs = G.truth_chain(500)
    cl, cr, ids, pairs = T.chimeras(starts, lens, strands, recs, count=40)
    G.check_records(cr, cl)
    assert all(abs(int(starts[a]) - int(starts[b])) > 30000 for a, b in pairs)
    c = T.clips(cr, cl, end_clip=500)
    assert np.all(c["nregions"][ids] >= 2) and not np.any(c["nregions"][:len(lens)] >= 2)
    c0 = T.clips(cr, cl, end_clip=0)
    assert not np.any(c0["nregions"][ids] >= 2)
    # the clip of a chimera is one of its two reads' stretches
    la = np.array([lens[a] for a, _ in pairs])
    assert np.all((c["end"][ids] <= la) | (c["beg"][ids] >= la))


def test_polish_through_the_clip():
    """the trimmed polish wrapper with whole-read clips is unitig_mirror.polished; with a clip it takes the decisions of the original
    positions"""
    starts, lens, strands, recs = G.truth_chain(30)
    seqs = U.reads_from_genome(U.random_genome(int((starts + lens).max()), 2), starts, lens, strands)
    whole = np.zeros(len(lens), T.CLIP_DT)
    whole["end"] = lens
    m = T.build(recs, lens, whole)
    assert m["records_outside"] == 0 and m["edges"].tobytes() == G.build(recs, lens)["edges"].tobytes()
    u = U.unitigs(m["offsets"], m["edges"], m["contained"], None, lens)
    table = U.random_table(lens, 0)
    a, b = T.polished(u, seqs, table, whole), U.polished(u, seqs, table)
    assert a["bases"] == b["bases"] and a["stats"].tobytes() == b["stats"].tobytes() and np.array_equal(a["pos"], b["pos"])
    jl, jr, head, tail = T.junk_ends(starts, lens, strands, recs, 0.5, 1200, 3000)
    jseqs = T.junk_seqs(seqs, head, tail)
    c = T.clips(jr, jl, end_clip=0)
    mj = T.build(jr, jl, c)
    dead = (mj["contained"] != 0).astype(np.uint8)
    uj = U.unitigs(mj["offsets"], mj["edges"], dead, None, mj["lens"])
    jt = U.random_table(jl, 1)
    p = T.polished(uj, jseqs, jt, c)
    v, n = int(uj["verts"][0]), int(uj["nbases"][0])
    r = v >> 1
    roff = int(np.sum(jl[:r]))
    d = U.decisions(jseqs[r], jt[roff:roff + int(jl[r])])
    idx = np.arange(int(c["end"][r]) - 1, int(c["end"][r]) - 1 - n, -1) if v & 1 else np.arange(int(c["beg"][r]), int(c["beg"][r]) + n)
    assert int(p["nbases"][0]) == int(d["keep"][idx].sum() + d["ins"][idx].sum())


def test_parameters():
    lens, recs = np.array([5000, 5000], np.int64), np.zeros(0, G.OVL_DT)
    assert T.clips(recs, lens).tolist() == [(0, 0, 0, 0)] * 2
    with pytest.raises(ValueError):
        T.clips(recs, lens, min_depth=0)
    with pytest.raises(TypeError):
        T.clips(recs, lens, fuzz=1)
    assert T.DEFAULTS == dict(api.Engine.TRIM_DEFAULTS) == dict(min_depth=3, end_clip=500, min_span=1000)


def test_trimmed_reads_on_the_host():
    seqs = [b"ACGTACGTAC", b"GGGG", b"TTTTTTCC", b""]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    bases = np.frombuffer(b"".join(seqs), np.uint8)
    clip = np.zeros(4, T.CLIP_DT)
    clip["beg"], clip["end"] = [2, 0, 6, 0], [7, 0, 8, 0]
    o, b = api.trimmed_reads(offs, bases, clip)
    assert o.dtype == np.uint64 and o.tolist() == [0, 5, 5, 7, 7] and b.tobytes() == b"GTACGCC"
    assert [b.tobytes()[int(o[i]):int(o[i + 1])] for i in range(4)] == T.clip_seqs(seqs, clip)
    assert T.trimmed_fasta_text(["a", "b", "c", "d"], seqs, clip) == b">a\nGTACG\n>c\nCC\n"


def test_trim_structs_equal_the_header_as_a_c_compiler_sees_them(tmp_path):
    structs = {"bella_graph_trim_params": _lib.GraphTrimParams, "bella_read_clip": _lib.ReadClip, "bella_trim_stats": _lib.TrimStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            src.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    for cname in ("bella_graph_params", "bella_graph_stats", "bella_graph_edge", "bella_overlap", "bella_unitig_stats", "bella_polish_stats"):
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
    src.append('printf("abi version %d\\n", BELLA_HIP_ABI_VERSION);')
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(_lib.GraphTrimParams) == 16 and ctypes.sizeof(_lib.ReadClip) == 16 == _lib.CLIP_DT.itemsize == T.CLIP_DT.itemsize and ctypes.sizeof(_lib.TrimStats) == 88
    assert _lib.CLIP_DT == T.CLIP_DT and [n for n, _ in _lib.ReadClip._fields_] == list(T.CLIP_DT.names)
    # additive: the version and the existing structs stay what they were
    assert got[("abi", "version")] == 6 and _lib.load().bella_hip_abi_version() == 6
    for cname, cls in (("bella_graph_params", _lib.GraphParams), ("bella_graph_stats", _lib.GraphStats), ("bella_unitig_stats", _lib.UnitigStats),
                       ("bella_polish_stats", _lib.PolishStats)):
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
    assert got[("bella_graph_edge", "size")] == 24 and got[("bella_overlap", "size")] == 32 and got[("bella_graph_params", "size")] == 20 and got[("bella_graph_stats", "size")] == 104


def test_cli_refuses_the_options_without_their_context():
    from bella_amd import build as b
    exe = b.build_cli()
    for flags, word in ((["--trim"], "--trim needs --gfa, --unitigs or --unitigs-fasta"), (["--trim-depth", "2"], "need --trim"), (["--trim-end-clip", "20", "--gfa", "g"], "need --trim"),
                        (["--trimmed-reads", "t.fa", "--unitigs", "u"], "need --trim"), (["--trim", "--gfa", "g", "--trim-depth", "0"], "at least 1"),
                        (["--trim", "--unitigs-fasta", "u", "--trim-end-clip", "-1"], "must not be negative"), (["--trim", "--gfa", "g", "--skip-alignment"], "--skip-alignment")):
        p = subprocess.run([exe, "-f", "none.txt", "-o", "none"] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and word in p.stderr.decode(), flags
