"""GPU tests of the traced alignments: bella_hip_trace_pairs / _batch against the numpy mirror of the
definition (bella_testkit/trace_mirror.py), the replay checker on every traced pair, and bella-hip --paf --cigar end to end."""
import gzip
import multiprocessing as mp
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib, api
from bella_testkit import synth
from bella_testkit import trace_mirror as M
from bella_testkit.pipeline import aligned as _aligned, run_cli
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu

COVER = 1 << 18          # a first band no rectangle exceeds: every side runs with the band that holds its rectangle
SAMPLE = 200             # pairs per set compared with the mirror (fixed seed); all of them where a set has fewer


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


_SEQS = None


def _mirror_job(job):
    rid, cid, sh, sv, k, a = job
    return M.trace_expect(_SEQS[rid], _SEQS[cid], sh, sv, k, a)


def _mirror(seqs, jobs):
    global _SEQS
    _SEQS = seqs
    # (forked workers inherit the parent's device file descriptors: 12 of them + the parent stay clear of a limit of 16 such processes)
    with mp.get_context("fork").Pool(min(12, os.cpu_count() or 1)) as pool:
        return pool.map(_mirror_job, jobs, chunksize=4)


def _check_all(seqs, pairs, alns, tr, ops, idx, k_of=17):
    """replay + counters + end points inside the X-drop's, for every pair of idx"""
    for n in idx:
        p, a, t = pairs[n], alns[n], tr[n]
        assert t["nops"] > 0, n
        M.check_trace(t, ops, seqs[int(p["rid"])], seqs[int(p["cid"])], int(a["strand"]))
        lh, k = len(seqs[int(p["rid"])]), int(k_of)
        sH = lh - int(p["seedH"]) - k if a["strand"] else int(p["seedH"])
        if a["begH"] <= sH and a["begV"] <= p["seedV"]:
            assert a["begH"] <= t["tbegH"] and a["begV"] <= t["tbegV"], (n, a, t)
        # (else: the reference overwrote the begin points with the reads' lengths, xavier.h:356-360: they bound nothing)
        assert 0 <= t["tbegH"] <= sH and sH + k <= t["tendH"] <= max(a["endH"], sH + k) and 0 <= t["tbegV"] <= p["seedV"] and p["seedV"] + k <= t["tendV"] <= max(a["endV"], p["seedV"] + k), (n, a, t)


def _sample(idx, seed):
    if len(idx) <= SAMPLE:
        return list(idx)
    return sorted(np.random.default_rng(seed).choice(idx, SAMPLE, replace=False).tolist())


def _jobs(pairs, alns, idx, k):
    return [(int(pairs[n]["rid"]), int(pairs[n]["cid"]), int(pairs[n]["seedH"]), int(pairs[n]["seedV"]), k,
             {f: int(alns[n][f]) for f in ("begH", "endH", "begV", "endV", "strand")}) for n in idx]


def test_cover_band_equals_the_mirror_and_default_band_never_exceeds_it(eng, golden):
    """every golden set, all passed pairs.  Band forced to cover: the ops replay, the counters agree with them, the end points lie
    inside the X-drop's, and score + end points equal the mirror's full-rectangle optimum exactly (a fixed-seed sample of 200 pairs
    where a set has more).  Default band: valid, and never above the optimum; widened pairs and pairs short of the optimum are
    printed (DESIGN.md section 9 records the shares).  Also printed: how trace.score relates to the X-drop's score."""
    g = golden
    pars, pairs, alns = _aligned(eng, g)
    passed = np.flatnonzero(alns["passed"]).tolist()
    tr, ops = eng.trace_pairs(pars, band0=COVER)
    assert int((tr["nops"] > 0).sum()) == len(passed) and all(tr["nops"][n] > 0 for n in passed)
    assert int(tr["nops"].sum()) == len(ops)
    _check_all(g.seqs, pairs, alns, tr, ops, passed, g.k)
    pick = _sample(passed, 11)
    exp = _mirror(g.seqs, _jobs(pairs, alns, pick, g.k))
    for n, e in zip(pick, exp):
        got = {f: int(tr[n][f]) for f in e}
        assert got == e, (g.name, n, got, e)
    st = eng.trace_stats()
    assert st.pairs == len(passed) and st.widened_extensions == 0
    # the X-drop's score against the traced one (not asserted: DESIGN.md section 9 says why)
    below = [n for n in passed if tr[n]["score"] < alns[n]["score"]]
    worst = max([int(alns[n]["score"]) - int(tr[n]["score"]) for n in below], default=0)
    print("TRACE %s: passed %d, mirror-checked %d, trace.score < xdrop.score on %d (flagged among them %d), worst gap %d"
          % (g.name, len(passed), len(pick), len(below), sum(int(alns[n]["flagged"]) for n in below), worst))
    # default band on the same pairs
    tr2, ops2 = eng.trace_pairs(pars)
    _check_all(g.seqs, pairs, alns, tr2, ops2, passed, g.k)
    short = 0
    for n in passed:
        assert tr2[n]["score"] <= tr[n]["score"], (g.name, n)          # never above the optimum of the definition
        short += int(tr2[n]["score"] < tr[n]["score"])
    st2 = eng.trace_stats()
    print("TRACE %s: default band %d: pairs widened %d of %d, extensions repeated %d, pairs short of the optimum %d"
          % (g.name, st2.band0, int((tr2["widened"] > 0).sum()), len(passed), st2.widened_extensions, short))
    # and the same bytes when it runs again
    tr3, ops3 = eng.trace_pairs(pars)
    assert tr3.tobytes() == tr2.tobytes() and ops3.tobytes() == ops2.tobytes()


def test_trace_needs_alignments_first():
    e = Engine(0)
    try:
        with pytest.raises(api.BellaHipError) as ex:
            e.trace_pairs(BellaPars())
        assert ex.value.code == -7                                       # BELLA_ERR_STATE
    finally:
        e.close()


def test_trace_batch_on_explicit_seeds(eng):
    """seeds that match, seeds that do not (their columns become X), seeds at the ends of the reads, both strands: trace_batch
    equals the mirror, and equals trace_pairs where the seeds are a context's own pairs"""
    g = load_golden("toy120")
    pars, pairs, alns = _aligned(eng, g)
    passed = np.flatnonzero(alns["passed"])[:40]
    tr, ops = eng.trace_pairs(pars, band0=COVER)
    seeds = np.zeros(len(passed), _lib.SEED_DT)
    for f in ("rid", "cid", "seedH", "seedV"):
        seeds[f] = pairs[f][passed]
    bt, bops = eng.trace_batch(seeds, alns[passed], pars, band0=COVER)
    for q, n in enumerate(passed):
        for f in ("nops", "band", "score", "tbegH", "tendH", "tbegV", "tendV", "n_eq", "n_x", "n_ins", "n_del"):
            assert bt[q][f] == tr[n][f], (q, f)
        assert np.array_equal(bops[int(bt[q]["op_off"]):int(bt[q]["op_off"]) + int(bt[q]["nops"])],
                              ops[int(tr[n]["op_off"]):int(tr[n]["op_off"]) + int(tr[n]["nops"])])
    # hand-made seeds: arbitrary positions (mostly not matching), seeds at both read ends, both strands, whole-read rectangles
    rng = np.random.default_rng(5)
    lens = g.rs.lengths
    k = g.k
    rows = []
    for q in range(60):
        rid, cid = int(rng.integers(1, g.rs.nreads)), int(rng.integers(0, g.rs.nreads))
        lh, lv = int(lens[rid]), int(lens[cid])
        sh = [0, lh - k, int(rng.integers(0, lh - k + 1))][q % 3]
        sv = [int(rng.integers(0, lv - k + 1)), 0, lv - k][q % 3]
        strand = q & 1
        sHo = lh - sh - k if strand else sh
        bH, bV = int(rng.integers(max(0, sHo - 300), sHo + 1)), int(rng.integers(max(0, sv - 300), sv + 1))
        eH, eV = int(rng.integers(sHo + k, min(lh, sHo + k + 300) + 1)), int(rng.integers(sv + k, min(lv, sv + k + 300) + 1))
        rows.append((rid, cid, sh, sv, strand, bH, eH, bV, eV))
    seeds = np.zeros(len(rows), _lib.SEED_DT)
    al = np.zeros(len(rows), _lib.ALN_DT)
    for q, (rid, cid, sh, sv, strand, bH, eH, bV, eV) in enumerate(rows):
        seeds[q] = (rid, cid, sh, sv)
        al[q]["begH"], al[q]["endH"], al[q]["begV"], al[q]["endV"], al[q]["strand"], al[q]["passed"] = bH, eH, bV, eV, strand, 1
    for band in (COVER, 0):
        bt, bops = eng.trace_batch(seeds, al, pars, band0=band)
        for q, (rid, cid, sh, sv, strand, bH, eH, bV, eV) in enumerate(rows):
            M.check_trace(bt[q], bops, g.seqs[rid], g.seqs[cid], strand)
            e = M.trace_expect(g.seqs[rid], g.seqs[cid], sh, sv, k, dict(begH=bH, endH=eH, begV=bV, endV=eV, strand=strand))
            if band == COVER:
                assert {f: int(bt[q][f]) for f in e} == e, (q, rows[q])
            else:
                assert bt[q]["score"] <= e["score"]
    assert int((bt["n_x"] > 0).sum()) > 0


def _parse_paf_cigar(data, seqs_by_name):
    """every line: 12 columns + AS ov NM cg; cg replays against the reads; columns 10/11 and NM agree with the ops"""
    lines = data.decode().splitlines()
    for ln in lines:
        c = ln.split("\t")
        assert len(c) == 16 and c[11] == "255" and c[12].startswith("AS:i:") and c[13].startswith("ov:i:") and c[14].startswith("NM:i:") and c[15].startswith("cg:Z:"), ln[:200]
        V, H = seqs_by_name[c[0]], seqs_by_name[c[5]]
        assert int(c[1]) == len(V) and int(c[6]) == len(H)
        ops = M.parse_cigar(c[15][5:])
        if c[4] == "-":           # H coordinates on the original strand, runs along H forwards: replay H forwards against revcomp(V), V backwards
            got = M.replay(ops, H, M.revcomp(V), int(c[7]), int(c[8]), len(V) - int(c[3]), len(V) - int(c[2]))
        else:
            got = M.replay(ops, H, V, int(c[7]), int(c[8]), int(c[2]), int(c[3]))
        assert int(c[9]) == got["n_eq"] and int(c[10]) == got["n_eq"] + got["n_x"] + got["n_ins"] + got["n_del"]
        assert int(c[14][5:]) == got["n_x"] + got["n_ins"] + got["n_del"]
    return lines


def _run(*args):
    return run_cli(*args)["out.out"]


@pytest.mark.parametrize("name", ["toy120", "toylen80"])
def test_cli_paf_cigar_end_to_end(name, tmp_path):
    """bella-hip --paf --cigar on two golden sets: every line parses, cg replays against the FASTQ, columns 10/11/NM match the ops,
    one line per line of the golden PAF with the same names and strand; without --cigar the file is still the golden paf.out"""
    g = load_golden(name)
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r + 1, k + 1, q) for k, r, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    base = g.meta["flags"] + ["--tuples", mtx, "--paf"]
    assert _run([fq], base, str(tmp_path / "plain")) == g.out["paf"]
    data = _run([fq], base + ["--cigar"], str(tmp_path / "cigar"))
    by_name = dict(zip(g.names, g.seqs))
    lines = _parse_paf_cigar(data, by_name)
    gold = g.out["paf"].decode().splitlines()
    assert len(lines) == len(gold)
    for a, b in zip(lines, gold):
        ca, cb = a.split("\t"), b.split("\t")
        assert (ca[0], ca[1], ca[4], ca[5], ca[6]) == (cb[0], cb[1], cb[4], cb[5], cb[6])
        assert ca[12] == "AS:i:" + cb[9] and ca[13] == "ov:i:" + cb[10]
        assert 0 <= int(ca[2]) < int(ca[3]) <= int(ca[1]) and 0 <= int(ca[7]) < int(ca[8]) <= int(ca[6])
    assert len(_parse_paf_cigar(_run([fq], base + ["--cigar", "--trace-band", "512"], str(tmp_path / "cigar512")), by_name)) == len(gold)


def test_cli_cigar_same_file_over_contexts_stages_and_twice(tmp_path):
    """--paf --cigar: two runs give identical bytes; -g 2 (two contexts on the one GPU), -m 1 (stages) and both give the plain run's
    file; --exact-xdrop --cigar replays as well"""
    rs = synth.make_reads(1200, read_len=3000, err=0.15, seed=78)
    fq = str(tmp_path / "a.fastq")
    synth.write_fastq(fq, rs)
    by_name = dict(zip(rs.names, rs.seqs()))
    over = {"BELLA_HIP_OVERSUBSCRIBE": "1"}
    base = _run([fq], ["--paf", "--cigar"], str(tmp_path / "base"))
    assert len(_parse_paf_cigar(base, by_name)) > 100
    assert _run([fq], ["--paf", "--cigar"], str(tmp_path / "again")) == base
    assert _run([fq], ["--paf", "--cigar", "-g", "2"], str(tmp_path / "g2"), over) == base
    assert _run([fq], ["--paf", "--cigar", "-m", "1"], str(tmp_path / "m1")) == base
    assert _run([fq], ["--paf", "--cigar", "-m", "1", "-g", "2"], str(tmp_path / "m1g2"), over) == base
    ex = _run([fq], ["--paf", "--cigar", "--exact-xdrop"], str(tmp_path / "exact"))
    assert len(_parse_paf_cigar(ex, by_name)) > 100
    assert _run([fq], ["--paf", "--cigar", "--exact-xdrop", "-m", "1"], str(tmp_path / "exact_m1")) == ex


def test_larger_synthetic_set_10kb_reads(eng):
    """2,000 reads of 10 kb at 15 % error (the case where the band matters): default band, every passed pair replays with the right
    counters; a fixed-seed sample of 200 pairs with the band forced to cover equals the mirror, and the default band's score on
    them never exceeds it"""
    rs = synth.make_reads(2000, read_len=10000, err=0.15, seed=21)
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    pairs, _, _ = eng.get_pairs()
    eng.align_pairs(pars)
    alns = eng.get_alignments()
    seqs = rs.seqs()
    passed = np.flatnonzero(alns["passed"]).tolist()
    assert len(passed) > 2000
    tr, ops = eng.trace_pairs(pars)
    st = eng.trace_stats()
    _check_all(seqs, pairs, alns, tr, ops, passed)
    pick = _sample(passed, 12)
    seeds = np.zeros(len(pick), _lib.SEED_DT)
    for f in ("rid", "cid", "seedH", "seedV"):
        seeds[f] = pairs[f][pick]
    bt, bops = eng.trace_batch(seeds, alns[pick], pars, band0=COVER)
    exp = _mirror(seqs, _jobs(pairs, alns, pick, 17))
    short = 0
    for q, (n, e) in enumerate(zip(pick, exp)):
        M.check_trace(bt[q], bops, seqs[int(pairs[n]["rid"])], seqs[int(pairs[n]["cid"])], int(alns[n]["strand"]))
        assert {f: int(bt[q][f]) for f in e} == e, (n, e)
        assert tr[n]["score"] <= e["score"]
        short += int(tr[n]["score"] < e["score"])
    print("TRACE synth 2000 x 10 kb: passed %d, default band %d: pairs widened %d, extensions repeated %d of %d, of %d sampled pairs %d short "
          "of the optimum; dp %.1f ms, walks %.1f ms, total %.1f ms, %.3g cells, %.3g direction bytes"
          % (len(passed), st.band0, int((tr["widened"] > 0).sum()), st.widened_extensions, st.extensions, len(pick), short, st.dp_ms, st.walk_ms,
             st.total_ms, st.dp_cells, st.dir_bytes))


def test_cli_cigar_with_no_candidate_pairs(tmp_path):
    """a handful of unrelated reads: no pair, no line -- with --paf --cigar as without, an empty file and exit 0; the same with a
    -m budget and with two contexts"""
    rng = np.random.default_rng(9)
    rs = synth.ReadSet.from_strings([bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1500).tolist()) for _ in range(6)])
    fq = str(tmp_path / "u.fastq")
    synth.write_fastq(fq, rs)
    assert _run([fq], ["--paf"], str(tmp_path / "plain")) == b""
    assert _run([fq], ["--paf", "--cigar"], str(tmp_path / "cigar")) == b""
    assert _run([fq], ["--paf", "--cigar", "-m", "1"], str(tmp_path / "m1")) == b""
    assert _run([fq], ["--paf", "--cigar", "-g", "2"], str(tmp_path / "g2"), {"BELLA_HIP_OVERSUBSCRIBE": "1"}) == b""


def test_cli_cigar_staged_run_that_starts_with_columns_without_pairs(tmp_path):
    """-m stages over a file whose first 40 reads are unrelated to everything (their columns hold no pair): the single-stage file"""
    rng = np.random.default_rng(10)
    junk = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000).tolist()) for _ in range(40)]
    rel = synth.make_reads(600, read_len=3000, err=0.15, seed=79)
    rs = synth.ReadSet.from_strings(junk + rel.seqs())
    fq = str(tmp_path / "j.fastq")
    synth.write_fastq(fq, rs)
    base = _run([fq], ["--paf", "--cigar"], str(tmp_path / "base"))
    assert len(base.splitlines()) > 50
    assert _run([fq], ["--paf", "--cigar", "-m", "1"], str(tmp_path / "m1")) == base
