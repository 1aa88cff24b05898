"""What the GPU tests of the stages after the alignment share: the way to aligned pairs, the overlap records of traced pairs, a stress
input for the graph, an error check, the runner of the command line, and the one of the ranks of a collective call."""
import os
import subprocess
import threading

import numpy as np
import pytest

from bella_amd import BellaPars, api
from bella_testkit import graph_mirror as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def aligned(eng, g):
    """a golden set's reads and tuples -> overlap -> alignment: (pars, pairs, alignments)"""
    eng.set_reads(g.rs)
    eng.assemble_tuples(g.k, g.nkmers, g.tk, g.tr, g.tp)
    pars = BellaPars(kmerSize=g.k, errorRate=g.err)
    eng.overlap(pars)
    pairs, _, _ = eng.get_pairs()
    eng.align_pairs(pars)
    return pars, pairs, eng.get_alignments()


def records(pairs, alns, tr):
    """the overlap records graph_add_traced makes of the passed, traced pairs"""
    m = (alns["passed"] == 1) & (tr["nops"] > 0)
    recs = np.zeros(int(m.sum()), G.OVL_DT)
    recs["cid"], recs["rid"] = pairs["cid"][m], pairs["rid"][m]
    for f, t in (("begV", "tbegV"), ("endV", "tendV"), ("begH", "tbegH"), ("endH", "tendH")):
        recs[f] = tr[t][m]
    recs["score"], recs["strand"] = alns["score"][m], alns["strand"][m]
    return recs


def hub_and_band(nreads=3000, hub=700, band=8, L=20000):
    """a 700-way fork at read 0 and an eight-wide band over the other reads: (records, lengths)"""
    out = []
    for j in range(1, hub + 1):
        out.append((0, j, L // 2 + j, L, 0, L // 2 - j, 0, j & 1, (0, 0, 0)))
    for i in range(1, nreads - band):
        for d in range(1, band + 1):
            out.append((i, i + d, 1000 * d, L, 0, L - 1000 * d, 0, (i + d) % 3 == 0, (0, 0, 0)))
    out.append((nreads - 2, nreads - 1, 0, L, 0, L, 0, 0, (0, 0, 0)))
    return np.array(out, G.OVL_DT), np.full(nreads, L, np.int64)


def raises(code, fn, *a, **kw):
    with pytest.raises(api.BellaHipError) as ex:
        fn(*a, **kw)
    assert ex.value.code == code, (fn, ex.value.code)


# ---- the rounds of DESIGN.md sections 18 to 20 under BELLA_TUNE_ROUND_BUDGET: the batching changes, the result does not
def with_round_budget(eng, budget, run):
    """run() with `budget` direction bytes per batch of a round (None: the default rule); the default rule again on every way out"""
    try:
        if budget is not None:
            eng.set_tuning("round_budget", budget)
        return run()
    finally:
        eng.set_tuning("round_budget")


def realign_getters(eng, **params):
    """one realignment round: what every getter returns afterwards, the stats (with `wrapped`) under "st" """
    out = dict(eng.graph_realign_unitigs(**params))
    out["placements"] = eng.realign_placements()
    out["ops"], out["table"] = eng.realign_ops()
    out["st"] = eng.realign_stats()
    return out


def recorrect_getters(eng, **params):
    """one correction round: what every getter returns afterwards, the stats under "st" """
    out = dict(zip(("offsets", "bases", "stats"), eng.recorrect(**params)))
    out["jobs"] = eng.recorrect_jobs()
    out["ops"], out["table"] = eng.recorrect_ops()
    out["anchor_offsets"], out["anchors"] = eng.recorrect_anchors()
    out["st"] = eng.recorrect_stats()
    return out


def same_but_for_the_batching(a, b):
    """two rounds' getters: every array equal in type, shape and every byte of every field (records with their op_off and nops), the
    stats in every field but the timers, `batches` and `dir_bytes_peak`"""
    assert a.keys() == b.keys()
    for k in a:
        if k == "st":
            skip = [f for f in a[k] if f.endswith("_ms") or f in ("batches", "dir_bytes_peak")]
            assert {f: v for f, v in a[k].items() if f not in skip} == {f: v for f, v in b[k].items() if f not in skip}
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        for f in a[k].dtype.names or [None]:
            assert (a[k] if f is None else a[k][f]).tobytes() == (b[k] if f is None else b[k][f]).tobytes(), (k, f)


def dps_and_largest_job(band, n, band0):
    """from the last band and the length of every job whose DP ran: (the DPs that ran -- a job whose last band is B ran log2(B / band0) + 1
    times --, the largest single job's direction bytes, n x B / 4)"""
    band, n = np.asarray(band, np.int64), np.asarray(n, np.int64)
    return int((np.log2(band // band0).astype(np.int64) + 1).sum()), int((n * band // 4).max())


def run_ranks(nranks, body, timeout=300):
    """one host thread per context (ctypes releases the GIL): the collective entry points rendezvous inside the library"""
    out, err = [None] * nranks, []

    def work(r):
        try:
            out[r] = body(r)
        except Exception as e:  # noqa: BLE001
            err.append((r, e))
    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert not any(t.is_alive() for t in th), "a rank is still inside a collective call: the ranks did not leave it together"
    return out, err


def run_cli(fastqs, flags, cwd, env_extra=None):
    """bella-hip -f <list of fastqs> -o out <flags> in `cwd`, which must succeed: {file name: bytes} of every file it left there (the
    -o file is "out.out"), and its log under "stderr" (bytes)"""
    exe = os.path.join(ROOT, "bella_amd", "bin", "bella-hip")
    os.makedirs(cwd, exist_ok=True)
    with open(os.path.join(cwd, "in.txt"), "w") as f:
        f.write("".join(p + "\n" for p in fastqs))
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([exe, "-f", "in.txt", "-o", "out"] + list(flags), cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    out = {n: open(os.path.join(cwd, n), "rb").read() for n in os.listdir(cwd) if n != "in.txt" and os.path.isfile(os.path.join(cwd, n))}
    out["stderr"] = p.stderr
    return out
