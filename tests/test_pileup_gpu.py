"""GPU tests of the read correction: the pileup table accumulated on the device from the traced alignments and
the consensus call, both EQUAL to the numpy mirror (bella_testkit/pileup_mirror.py) applied to the device's own traces -- which
tests/test_trace_gpu.py pins to the trace mirror -- and bella-hip --correct end to end."""
import gzip
import multiprocessing as mp
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib, api
from bella_testkit import pileup_mirror as P
from bella_testkit import synth
from bella_testkit import trace_mirror as M
from bella_testkit.pipeline import aligned as _aligned, run_cli
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)


def test_table_equals_the_mirror_exactly(eng, golden):
    """every golden set: align -> trace with pileup, runs kept: the device's (bases, 9) table is the mirror's, built from the returned
    traces and ops.  The same without keeping the runs: identical table, no run staged on the host, the same records.  The table
    accumulates over calls until the next reset; read ranges and add_pileup address the same rows."""
    g = golden
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    tr, ops = eng.trace_pairs(pars, pileup=True, keep_ops=True)
    st = eng.trace_stats()
    table = eng.get_pileup()
    nb = int(sum(len(s) for s in g.seqs))
    assert table.shape == (nb, 9) and table.dtype == np.uint32 and eng.pileup_bytes() == 36 * nb
    want, dropped = P.pileup(g.seqs, pairs, alns, tr, ops)
    assert np.array_equal(table, want), (g.name, np.argwhere(table != want)[:5])
    assert st.votes == int(want.sum(dtype=np.int64)) and st.ops_host_bytes == 4 * len(ops) and st.ops == len(ops)
    # the traces are what bella_hip_trace_pairs gives
    tr0, ops0 = eng.trace_pairs(pars)
    assert tr0.tobytes() == tr.tobytes() and ops0.tobytes() == ops.tobytes()
    # without the runs on the host
    eng.pileup_reset()
    assert int(eng.get_pileup().sum(dtype=np.int64)) == 0
    tr2, ops2 = eng.trace_pairs(pars, pileup=True, keep_ops=False)
    st2 = eng.trace_stats()
    assert len(ops2) == 0 and st2.ops_host_bytes == 0 and st2.ops == len(ops) and st2.votes == st.votes
    assert tr2.tobytes() == tr.tobytes()
    assert np.array_equal(eng.get_pileup(), want)
    with pytest.raises(api.BellaHipError) as ex:                     # the runs were not kept: only the records are handed out
        buf = np.zeros(max(len(ops), 1), np.uint32)
        eng._chk(eng.lib.bella_hip_get_traces(eng.h, None, buf.ctypes.data))
    assert ex.value.code == -7
    print("PILEUP %s: pairs %d, runs %d, votes %d (dropped %d), vote %.3f ms, walks %.3f ms, dp %.3f ms"
          % (g.name, st.pairs, st.ops, st.votes, dropped, st2.vote_ms, st2.walk_ms, st2.dp_ms))
    # accumulation, ranges, add
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    assert np.array_equal(eng.get_pileup(), 2 * want)
    off = _offsets(g.seqs)
    a, n = g.rs.nreads // 3, g.rs.nreads // 2
    part = eng.get_pileup(a, n)
    assert np.array_equal(part, 2 * want[off[a]:off[a + n]])
    eng.add_pileup(a, n, part)
    exp = 2 * want.astype(np.int64)
    exp[off[a]:off[a + n]] *= 2
    assert np.array_equal(eng.get_pileup().astype(np.int64), exp)


def test_consensus_equals_the_mirror_exactly(eng, golden):
    """Engine.consensus against the mirror's consensus on the device's table: bases and statistics of every read, for min_depth 1, 3
    and 1,000,000 (which returns every read unchanged)"""
    g = golden
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    table = eng.get_pileup()
    off = _offsets(g.seqs)
    for md in (1, 3, 1000000):
        offs, bases, stats = eng.consensus(md)
        assert offs[0] == 0 and int(offs[-1]) == len(bases) and len(stats) == g.rs.nreads
        raw = bases.tobytes()
        changed = 0
        for r, s in enumerate(g.seqs):
            seq, want = P.consensus(s, table[off[r]:off[r + 1]], md)
            got = raw[int(offs[r]):int(offs[r + 1])]
            assert got == seq, (g.name, md, r)
            assert {f: int(stats[r][f]) for f in want} == want, (g.name, md, r)
            changed += got != s
            if md == 1000000:
                assert got == s
        print("CONSENSUS %s min_depth %d: %d of %d reads changed, %d -> %d bases, substituted %d, deleted %d, inserted %d"
              % (g.name, md, changed, g.rs.nreads, int(stats["len_before"].sum()), int(stats["len_after"].sum()), int(stats["substituted"].sum()),
                 int(stats["deleted"].sum()), int(stats["inserted"].sum())))


def test_pileup_call_order_and_arguments():
    e = Engine(0)
    try:
        g = load_golden("sanity3")
        pars, _, _ = _aligned(e, g)
        with pytest.raises(api.BellaHipError) as ex:                 # no table yet
            e.trace_pairs(pars, pileup=True)
        assert ex.value.code == -7
        with pytest.raises(api.BellaHipError) as ex:
            e.consensus(3)
        assert ex.value.code == -7
        e.pileup_reset()
        with pytest.raises(api.BellaHipError) as ex:
            e.consensus(0)
        assert ex.value.code == -3
        offs, bases, stats = e.consensus(3)                          # an empty table: every read unchanged
        assert bases.tobytes() == b"".join(g.seqs) and int(stats["covered"].sum()) == 0
        with pytest.raises(api.BellaHipError) as ex:
            e._chk(e.lib.bella_hip_get_pileup(e.h, 1, g.rs.nreads, None))
        assert ex.value.code == -3
        e.set_reads(g.rs)                                            # other reads: the table goes with the old ones
        assert e.pileup_bytes() == 0
        with pytest.raises(api.BellaHipError) as ex:
            e.get_pileup()
        assert ex.value.code == -7
    finally:
        e.close()


def test_every_column_votes_twice_every_gap_base_once_every_gap_run_once(eng):
    """counting, on one golden set, from the records and the ops alone: sum(table) = 2 sum(n_eq + n_x) + runs of I + runs of D +
    sum(n_ins + n_del) - the votes for a junction behind a read's last base"""
    g = load_golden("toyjunk220")
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    tr, ops = eng.trace_pairs(pars, pileup=True)
    total = int(eng.get_pileup().sum(dtype=np.int64))
    t = tr[tr["nops"] > 0]
    assert len(t) > 100
    expect = 2 * int(t["n_eq"].astype(np.int64).sum() + t["n_x"].astype(np.int64).sum()) + int(t["n_ins"].astype(np.int64).sum() + t["n_del"].astype(np.int64).sum())
    runs_i = runs_d = dropped = 0
    for n in np.flatnonzero(tr["nops"] > 0):
        w = ops[int(tr[n]["op_off"]):int(tr[n]["op_off"]) + int(tr[n]["nops"])].astype(np.int64)
        ln, op = w >> 4, w & 15
        i = int(tr[n]["tbegV"]) + np.cumsum(np.where(op != 3, ln, 0)) - np.where(op != 3, ln, 0)
        j = int(tr[n]["tbegH"]) + np.cumsum(np.where(op != 2, ln, 0)) - np.where(op != 2, ln, 0)
        lenH, lenV = len(g.seqs[int(pairs[n]["rid"])]), len(g.seqs[int(pairs[n]["cid"])])
        runs_i += int((op == 2).sum())
        runs_d += int((op == 3).sum())
        dropped += int(((op == 3) & (i == lenV)).sum())              # V lacks the run, behind V's last base
        dropped += int(((op == 2) & (j == (0 if alns[n]["strand"] else lenH))).sum())       # H lacks it, behind H's last base (strand 1: before H' 0)
    assert total == expect + runs_i + runs_d - dropped, (total, expect, runs_i, runs_d, dropped)
    assert eng.trace_stats().votes == total
    print("COUNTING %s: %d votes = 2 x %d columns + %d gap bases + %d I runs + %d D runs - %d dropped"
          % (g.name, total, int(t["n_eq"].sum() + t["n_x"].sum()), int(t["n_ins"].sum() + t["n_del"].sum()), runs_i, runs_d, dropped))


# ---- command line ----------------------------------------------------------------------------------------------------------------
def _run(*args):
    files = run_cli(*args)
    return files["out.out"], files.get("c.fasta")


def _fasta(names, seqs):
    return b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in zip(names, seqs))


@pytest.mark.parametrize("name", ["toy120", "toylen80"])
def test_cli_correct_end_to_end(name, eng, tmp_path):
    """bella-hip --correct on two golden sets: the FASTA is the Python path's byte for byte; a second run, -m 1 (stages), -g 2 (two
    contexts on the one GPU) and both give the same FASTA; with --paf --cigar --correct the PAF is the --paf --cigar run's; the -o file
    is what it is without --correct; --min-depth reaches the consensus"""
    g = load_golden(name)
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    want = {}
    for md in (3, 1):
        offs, bases, _ = eng.consensus(md)
        f = str(tmp_path / ("py%d.fasta" % md))
        api.write_fasta(f, g.names, offs, bases)
        want[md] = open(f, "rb").read()
    assert want[3] != _fasta(g.names, g.seqs) and want[1] != want[3]           # (the sets have something to correct)
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r + 1, k + 1, q) for k, r, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    base = g.meta["flags"] + ["--tuples", mtx]
    over = {"BELLA_HIP_OVERSUBSCRIBE": "1"}
    cor = ["--correct", "c.fasta"]
    out0, none = _run([fq], base, str(tmp_path / "plain"))
    assert none is None and out0 == g.out["align"]
    out1, fa1 = _run([fq], base + cor, str(tmp_path / "cor"))
    assert fa1 == want[3] and out1 == out0
    assert _run([fq], base + cor, str(tmp_path / "again")) == (out0, fa1)
    assert _run([fq], base + cor + ["-m", "1"], str(tmp_path / "m1")) == (out0, fa1)
    assert _run([fq], base + cor + ["-g", "2"], str(tmp_path / "g2"), over) == (out0, fa1)
    assert _run([fq], base + cor + ["-m", "1", "-g", "2"], str(tmp_path / "m1g2"), over) == (out0, fa1)
    assert _run([fq], base + cor + ["--min-depth", "1"], str(tmp_path / "md1")) == (out0, want[1])
    paf0, _ = _run([fq], base + ["--paf"], str(tmp_path / "paf"))
    assert paf0 == g.out["paf"]
    assert _run([fq], base + ["--paf"] + cor, str(tmp_path / "pafcor")) == (paf0, fa1)
    cg, _ = _run([fq], base + ["--paf", "--cigar"], str(tmp_path / "cigar"))
    assert _run([fq], base + ["--paf", "--cigar"] + cor, str(tmp_path / "cigarcor")) == (cg, fa1)
    assert _run([fq], base + ["--paf", "--cigar", "-g", "2", "-m", "1"] + cor, str(tmp_path / "cigarcorg2"), over) == (cg, fa1)


def test_cli_correct_with_no_candidate_pairs(tmp_path):
    """a handful of unrelated reads: no pair votes, the FASTA holds the input reads -- also under a -m budget and with two contexts"""
    rng = np.random.default_rng(9)
    rs = synth.ReadSet.from_strings([bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1500).tolist()) for _ in range(6)])
    fq = str(tmp_path / "u.fastq")
    synth.write_fastq(fq, rs)
    want = _fasta(rs.names, rs.seqs())
    assert _run([fq], ["--correct", "c.fasta"], str(tmp_path / "a")) == (b"", want)
    assert _run([fq], ["--correct", "c.fasta", "-m", "1"], str(tmp_path / "m1")) == (b"", want)
    assert _run([fq], ["--correct", "c.fasta", "-g", "2"], str(tmp_path / "g2"), {"BELLA_HIP_OVERSUBSCRIBE": "1"}) == (b"", want)


# ---- does it correct? ---------------------------------------------------------------------------------------------------------------
def _dist(job):
    return P.edit_distance(job[0], job[1])


def test_it_corrects_10kb_reads_at_15_percent_error(eng):
    """2,000 synthetic reads of 10 kb at 15 % error, 30x (the set tests/test_trace_gpu.py traces).  Read names carry start, length and
    strand and the genome is the generator's first draw from its seed, so every read's true template is known.  A fixed-seed sample of
    40 interior reads (start at least one read length from either genome end) whose positions with depth >= min_depth are at least
    half the read: global edit distance to the template, raw and corrected (min_depth 3).  Condition: the corrected sum is BELOW the raw
    sum.  Measured on an MI355X: all 40 drawn reads kept, raw 55,444 (13.86 % of the template bases), corrected
    15,186 (3.80 %), ratio 0.274."""
    nreads, read_len, seed, md = 2000, 10000, 21, 3
    rs = synth.make_reads(nreads, read_len=read_len, err=0.15, seed=seed)
    G = max(read_len + 1, round(nreads * read_len / 30.0))
    genome = np.random.default_rng(seed).integers(0, 4, size=G, dtype=np.uint8)
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    npass = eng.align_pairs(pars)
    assert npass > 2000
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    st = eng.trace_stats()
    assert st.ops_host_bytes == 0 and st.votes > 0
    offs, bases, stats = eng.consensus(md)
    seqs = rs.seqs()
    meta = [tuple(int(x) for x in n.split("_")[1:]) for n in rs.names]                   # (start, length, strand)
    interior = [r for r, (s, L, _) in enumerate(meta) if s >= read_len and s + L <= G - read_len]
    drawn = sorted(np.random.default_rng(31).choice(interior, 40, replace=False).tolist())
    kept = [r for r in drawn if 2 * int(stats[r]["covered"]) >= int(stats[r]["len_before"])]
    assert 2 * len(kept) >= len(drawn), (len(kept), len(drawn))
    raw = bases.tobytes()
    jobs = []
    for r in kept:
        s, L, strand = meta[r]
        t = synth.BASES[genome[s:s + L]].tobytes()
        if strand:
            t = M.revcomp(t)
        jobs.append((seqs[r], t))
        jobs.append((raw[int(offs[r]):int(offs[r + 1])], t))
    # (forked workers inherit the parent's device file descriptors: 8 of them + the parent stay clear of a limit of 16 such processes)
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        d = pool.map(_dist, jobs, chunksize=1)
    d_raw, d_cor = sum(d[0::2]), sum(d[1::2])
    tlen = sum(len(j[1]) for j in jobs[0::2])
    print("CORRECTION 2000 x 10 kb, 15 %% error, min_depth %d: %d of %d drawn reads kept (left out %d); edit distance to the template raw %d (%.2f %%), "
          "corrected %d (%.2f %%), ratio %.3f; mean depth %.1f; substituted %d, deleted %d, inserted %d over all reads; vote %.1f ms, walks %.1f ms, dp %.1f ms, votes %d"
          % (md, len(kept), len(drawn), len(drawn) - len(kept), d_raw, 100.0 * d_raw / tlen, d_cor, 100.0 * d_cor / tlen, d_cor / d_raw,
             float(stats["depth_sum"].sum()) / float(stats["len_before"].sum()), int(stats["substituted"].sum()), int(stats["deleted"].sum()),
             int(stats["inserted"].sum()), st.vote_ms, st.walk_ms, st.dp_ms, st.votes))
    assert d_cor < d_raw, (d_cor, d_raw)
