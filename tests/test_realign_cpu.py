"""CPU tests of the realignment round: the mirror (bella_testkit/realign_mirror.py) against a plain full-matrix
DP and against a replay of its own runs, the placement cases by hand, one round on a layout built from truth, the case list of the GPU
tests, the new structs against the header and the command line's argument errors.  The device is held to this mirror in
test_realign_gpu.py."""
import ctypes
import os
import subprocess

import numpy as np

from bella_amd import _lib
from bella_testkit import graph_mirror as G
from bella_testkit import pileup_mirror as P
from bella_testkit import realign_cases as RC
from bella_testkit import realign_mirror as R
from bella_testkit import trace_mirror as T
from bella_testkit import unitig_mirror as U
from conftest import ROOT


def _noisy(template: bytes, rng, err=0.15, mix=(0.10, 0.60, 0.30)):
    """a read of `template` at the generator's error mix: (read, cum) with cum[t] = bases of the read in front of template base t"""
    out, cum = [], [0]
    p_sub, p_ins, p_del = (err * m for m in mix)
    for ch in template:
        x = rng.random()
        if x >= p_del:
            out.append(b"ACGT"[(b"ACGT".index(ch) + rng.integers(1, 4)) & 3] if x < p_del + p_sub else ch)
            if p_del + p_sub <= x < p_del + p_sub + p_ins:
                out.append(b"ACGT"[rng.integers(0, 4)])
        cum.append(len(out))
    return bytes(out), cum


def test_a_covering_band_gives_the_full_matrix_score_and_the_runs_replay():
    rng = np.random.default_rng(5)
    for k in range(12):
        m = int(rng.integers(50, 301))
        utg = U.random_genome(m, 300 + k)
        a = int(rng.integers(0, m // 2))
        read, _ = _noisy(utg[a:a + int(rng.integers(min(50, m - a), m - a + 1))], rng)
        if k % 3 == 2:
            read = U.random_genome(int(rng.integers(50, 301)), 400 + k)          # nothing in common
        res = R.semiglobal_banded(read[:300], utg, 0, 1024)                     # |q - i| < 512 holds in the whole rectangle
        read = read[:300]
        score, q_end = R.semiglobal_full(read, utg)
        assert (res["score"], res["q_end"]) == (score, q_end) and not res["touch"]
        got = R.replay(T.run_lengths(res["ops"]), read, utg, res["q_begin"], res["q_end"])
        assert got["score"] == score and got["n_eq"] + got["n_x"] + got["n_ins"] == len(read)
        narrow = R.semiglobal_banded(read, utg, a, 64)                          # a narrow band around the true diagonal: never better
        assert narrow["ops"] is None or narrow["score"] <= score


def test_a_band_without_a_reachable_end_counts_as_touched():
    utg, read = U.random_genome(100, 1), U.random_genome(400, 2)
    assert R.semiglobal_banded(read, utg, 0, 64) == dict(touch=True, ops=None)      # row 400 has no column <= 100 within 32 diagonals


def test_the_four_placement_cases_by_hand():
    """L_b = 100, L_c = 40, the numbers of the mirror's docstring; then each case on a unitig with o = 0 and o = 1, with and without clips"""
    rec = lambda cid, rid, bV, bH, t: np.array([(cid, rid, bV, bV + 10, bH, bH + 10, 0, t, (0, 0, 0))], G.OVL_DT)[0]
    assert R.anchor_frame(rec(7, 9, 30, 5, 0), 9, 100, 40) == (7, 25, 0)             # b = V, strand 0
    assert R.anchor_frame(rec(7, 9, 30, 5, 1), 9, 100, 40) == (7, 25, 1)             # b = V, strand 1
    assert R.anchor_frame(rec(9, 7, 10, 50, 0), 9, 100, 40) == (7, 40, 0)            # b = H', strand 0
    assert R.anchor_frame(rec(9, 7, 10, 50, 1), 9, 100, 40) == (7, 20, 1)            # b = H', strand 1
    # the backbone read's whole read starts at x0_b = 1000
    assert R.on_unitig(1000, 0, 25, 0, 100, 40) == (1025, 0) and R.on_unitig(1000, 0, 25, 1, 100, 40) == (1025, 1)
    assert R.on_unitig(1000, 1, 25, 0, 100, 40) == (1035, 1) and R.on_unitig(1000, 1, 25, 1, 100, 40) == (1035, 0)      # 100 - 25 - 40 = 35
    assert R.on_unitig(1000, 0, 20, 1, 100, 40) == (1020, 1) and R.on_unitig(1000, 1, 20, 1, 100, 40) == (1040, 0)
    # clips: the vertex's pos is where the CLIP starts, the whole read starts lead_b in front of it
    assert R.lead(10, 90, 100, 0) == 10 and R.lead(10, 90, 100, 1) == 10 and R.lead(10, 70, 100, 1) == 30 and R.lead(0, 100, 100, 1) == 0
    # place(): one backbone read 0 (length 100) at pos 0 with orientation o, one contained read 1 (length 40), every case, clipped or not
    for o in (0, 1):
        for clipped in (False, True):
            clips = (np.array([10, 5]), np.array([70, 35])) if clipped else None
            bb, be = (10, 70) if clipped else (0, 100)
            cb, ce = (5, 35) if clipped else (0, 40)
            u = dict(voff=np.array([0, 1], np.uint64), verts=np.array([o], np.uint32), pos=np.array([0], np.uint64), nbases=np.array([be - bb], np.uint32),
                     len=np.array([be - bb], np.uint64))
            cur = dict(offsets=np.array([0, be - bb], np.uint64), pos=u["pos"], nbases=u["nbases"])
            for r, (d, s) in ((rec(0, 1, 30, 5, 0), (25, 0)), (rec(0, 1, 30, 5, 1), (25, 1))):
                pl, cnt = R.place(u, cur, [100, 40], np.array([r]), [0, 1], [0, 0], clips, band0=256)
                x0b = -R.lead(bb, be, 100, o)
                x0, oc = (x0b + 100 - d - 40, s ^ 1) if o else (x0b + d, s)
                x = x0 + R.lead(cb, ce, 40, oc)
                assert (int(pl[1]["s"]), int(pl[1]["e"]), int(pl[1]["orient"]), int(pl[1]["anchor"])) == (x, x + ce - cb, oc, 0), (o, clipped, d, s)
                assert (int(pl[0]["s"]), int(pl[0]["e"]), int(pl[0]["orient"])) == (0, be - bb, o) and cnt["backbone"] == 1 and cnt["contained"] == 1


def test_raw_to_current_coordinates():
    pos, nb, cpos, cnb = np.array([0, 100, 250]), np.array([100, 150, 50]), np.array([0, 90, 240]), np.array([90, 150, 55])
    f = lambda x: R.to_current(x, pos, nb, cpos, cnb, 300, 295)
    assert [f(x) for x in (-7, 0, 50, 99, 100, 249, 250, 299, 300, 310)] == [-7, 0, 45, 89, 90, 239, 240, 240 + 49 * 55 // 50, 295, 305]


def test_one_round_corrects_a_layout_built_from_truth():
    """A 6 kb genome, reads of 1.5 kb at 15 % error and 30 x, a backbone chosen from the true positions, its unitig polished with the
    existing mirrors from extensions anchored at the true overlap starts.  Windows of 400 bases from every backbone segment's start against
    their templates: one realignment round brings the sum below the polished one."""
    rng = np.random.default_rng(77)
    glen, L, W = 6000, 1500, 400
    genome = U.random_genome(glen, 78)
    n = 30 * glen // L
    starts = np.sort(np.concatenate([[0, glen - L], rng.integers(0, glen - L + 1, n - 2)]))
    strands = rng.integers(0, 2, n)
    fwd, cums = zip(*(_noisy(genome[s:s + L], rng) for s in starts.tolist()))
    seqs = [T.revcomp(f) if o else f for f, o in zip(fwd, strands.tolist())]
    chain = [0]
    while starts[chain[-1]] + L < glen:
        chain.append(max(r for r in range(n) if starts[r] <= starts[chain[-1]] + L - 500))
    assert chain[-1] == n - 1 and len(chain) >= 5
    nb = [cums[a][starts[b] - starts[a]] for a, b in zip(chain, chain[1:])] + [len(fwd[chain[-1]])]
    u = dict(voff=np.array([0, len(chain)], np.uint64), verts=np.array([2 * r + int(strands[r]) for r in chain], np.uint32),
             pos=np.array(np.concatenate([[0], np.cumsum(nb)[:-1]]), np.uint64), nbases=np.array(nb, np.uint32), len=np.array([sum(nb)], np.uint64))
    # every read against every backbone read it shares >= 500 template bases with: an extension from the true start of the overlap
    pairs, alns, traces, ops, recs = [], [], [], [], []
    for b in chain:
        for x in range(n):
            lo, hi = max(starts[b], starts[x]), min(starts[b], starts[x]) + L
            if x == b or hi - lo < 500 or (x in chain and x < b):
                continue
            v, h = min(b, x), max(b, x)
            if strands[v] == 0:
                tv, th = cums[v][lo - starts[v]], cums[h][lo - starts[h]]
            else:
                tv, th = len(fwd[v]) - cums[v][hi - starts[v]], len(fwd[h]) - cums[h][hi - starts[h]]
            st = int(strands[v] ^ strands[h])
            Hp = T.oriented(seqs[h], st)
            score, (i, j), o, _ = T.banded_extension(Hp[th:], seqs[v][tv:], 256)
            runs = T.run_lengths(o[::-1])
            pairs.append((h, v)); alns.append(st); traces.append((len(runs), sum(len(q) for q in ops), tv, th))
            ops.append(runs)
            recs.append((v, h, tv, tv + i, th, th + j, score, st, (0, 0, 0)))
    pairs = np.array(pairs, [("rid", "<u4"), ("cid", "<u4")])
    alns = np.array(alns, [("strand", "<u4")])
    traces = np.array(traces, [("nops", "<u4"), ("op_off", "<u8"), ("tbegV", "<i4"), ("tbegH", "<i4")])
    table, _ = P.pileup(seqs, pairs, alns, traces, np.concatenate(ops))
    recs = np.array(recs, G.OVL_DT)
    pol = U.polished(u, seqs, table, 3)
    contained = np.array([0 if r in chain else 1 for r in range(n)], np.uint8)
    rea = R.realign_round(u, pol, seqs, recs, contained, np.zeros(n, np.uint8), None, band0=256)
    raw = U.unitig_bases(u, seqs)[1]
    d = [0, 0, 0]
    for i, r in enumerate(chain[:-1]):
        t = genome[starts[r]:starts[r] + 5 * W // 4]
        for k, (seq, at) in enumerate(((raw, u["pos"]), (pol["bases"], pol["pos"]), (rea["bases"], rea["pos"]))):
            d[k] += U.window_distance(seq[int(at[i]):int(at[i]) + W], t)
    print("REALIGN mirror, 6 kb genome, %d reads of 1.5 kb at 15 %%: %d backbone reads, %d windows of %d: raw %d, polished %d, realigned %d; %s"
          % (n, len(chain), len(chain) - 1, W, d[0], d[1], d[2], rea["counts"]))
    assert rea["counts"]["voted"] > n // 2
    assert d[2] < d[1] < d[0], d


def test_the_synthetic_lines_cover_what_the_gpu_tests_need():
    """the statuses of realign_cases.line_case under the three band settings and of the circle, from the mirrors alone"""
    seqs, recs = RC.line_case()
    m, c, u = U.case_unitigs(seqs, recs, RC.GRAPH, {})
    assert u["len"].tolist() == [6800, 900] and u["verts"].tolist() == [2, 7, 10, 15, 18, 28]
    p = U.polished(u, seqs, RC.line_table(seqs), 3)
    a = R.realign_round(u, p, seqs, recs, m["contained"], c["removed"], None, band0=256, band_max=2048)["placements"]
    assert a["status"].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, R.UNPLACED, 1, R.OUTSIDE, 1, 1, R.LOW_IDENTITY, 1] and a["band"][11] == 512
    assert a["q_begin"][0] == 0 and a["q_end"][4] == int(p["offsets"][1]) and a["orient"][0] == 1
    both = [x for x, r in enumerate(recs) if 2 in (int(r["cid"]), int(r["rid"])) and {int(r["cid"]), int(r["rid"])} & set(RC.BACKBONE)]
    assert len(both) == 2 and a["anchor"][2] == both[0] and int(recs[both[0]]["cid"]) == 1
    assert int(recs[int(a["anchor"][0])]["cid"]) == 0 and int(recs[int(a["anchor"][0])]["strand"]) == 1
    b = R.realign_round(u, p, seqs, recs, m["contained"], c["removed"], None, band0=512, band_max=512)["placements"]
    assert b["status"][12] == R.BAND_CAPPED and b["status"][11] == R.VOTED
    seqs, recs = RC.circle_case()
    m, c, u = U.case_unitigs(seqs, recs, RC.GRAPH, {})
    p = U.polished(u, seqs, np.zeros((sum(map(len, seqs)), 9), np.uint32), 3)
    r = R.realign_round(u, p, seqs, recs, m["contained"], c["removed"], None, band0=256)
    assert u["circular"].tolist() == [1] and (r["placements"]["status"] == R.OUTSIDE).sum() == 2 and r["bases"] == p["bases"]


def test_realign_structs_equal_the_header_as_a_c_compiler_sees_them(tmp_path):
    structs = {"bella_realign_params": _lib.RealignParams, "bella_realign_stats": _lib.RealignStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bella_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            src.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    src.append('printf("bella_realign_placement size %zu\\n", sizeof(bella_realign_placement));')
    for fname in _lib.PLACE_DT.names:
        src.append('printf("bella_realign_placement %s %%zu\\n", offsetof(bella_realign_placement, %s));' % (fname, fname))
    for cname in ("bella_polish_params", "bella_polish_stats", "bella_polish_unitig"):
        src.append('printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
    src.append('printf("abi version %d\\n", BELLA_HIP_ABI_VERSION);')
    src.append('printf("status values %d\\n", BELLA_REALIGN_NONE + 10 * BELLA_REALIGN_VOTED + 100 * BELLA_REALIGN_UNPLACED + 1000 * BELLA_REALIGN_OUTSIDE + 10000 * BELLA_REALIGN_BAND_CAPPED + 100000 * BELLA_REALIGN_LOW_IDENTITY);')
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", exe])
    protos = tmp_path / "protos.c"                                    # the prototypes, as a C compiler reads them (compiled, not linked)
    protos.write_text('#include "bella_hip.h"\n'
                      'int (*run)(bella_ctx*, const bella_realign_params*, uint64_t*) = bella_hip_graph_realign_unitigs;\n'
                      'int (*get)(bella_ctx*, uint64_t*, uint8_t*, uint64_t*, uint32_t*, bella_polish_unitig*) = bella_hip_graph_get_realigned;\n'
                      'int (*pl)(bella_ctx*, bella_realign_placement*) = bella_hip_graph_get_realign_placements;\n'
                      'int (*ops)(bella_ctx*, uint64_t*, uint32_t*, uint32_t*) = bella_hip_graph_get_realign_ops;\n'
                      'int (*st)(bella_ctx*, void*, uint64_t) = bella_hip_graph_get_realign_stats;\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(protos), "-o", str(tmp_path / "protos.o")])
    got = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        a, b, v = ln.split()
        got[(a, b)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert got[("bella_realign_placement", "size")] == _lib.PLACE_DT.itemsize == R.PLACE_DT.itemsize == 88
    for fname in _lib.PLACE_DT.names:
        assert got[("bella_realign_placement", fname)] == _lib.PLACE_DT.fields[fname][1] == R.PLACE_DT.fields[fname][1], fname
    assert ctypes.sizeof(_lib.RealignParams) == 24 and ctypes.sizeof(_lib.RealignStats) == 176
    assert got[("status", "values")] == 543210 and (R.NONE, R.VOTED, R.UNPLACED, R.OUTSIDE, R.BAND_CAPPED, R.LOW_IDENTITY) == tuple(range(6))
    assert (_lib.REALIGN_NONE, _lib.REALIGN_LOW_IDENTITY) == (0, 5)
    # additive: the version and the neighbouring structs stay what they were
    assert got[("abi", "version")] == 6 and _lib.load().bella_hip_abi_version() == 6
    assert got[("bella_polish_params", "size")] == ctypes.sizeof(_lib.PolishParams) == 8 and got[("bella_polish_stats", "size")] == ctypes.sizeof(_lib.PolishStats)
    assert got[("bella_polish_unitig", "size")] == _lib.POLISH_DT.itemsize == 56


def _cli():
    from bella_amd import build as b
    return b.build_cli()


def test_cli_help_lists_the_options():
    p = subprocess.run([_cli(), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0
    for opt in ("--polish-rounds arg", "--realign-band arg", "--realign-min-identity arg"):
        assert opt in p.stdout.decode(), opt


def test_cli_refuses_the_options_without_polish_and_out_of_range():
    """all of these are decided before a device is looked for"""
    need = "need --polish"
    for flags, word in ((["--unitigs", "u", "--polish-rounds", "2"], need), (["--unitigs", "u", "--realign-band", "512"], need),
                        (["--unitigs", "u", "--realign-min-identity", "600"], need),
                        (["--unitigs", "u", "--polish", "--polish-rounds", "0"], "--polish-rounds must be in [1, 4]"),
                        (["--unitigs", "u", "--polish", "--polish-rounds", "5"], "--polish-rounds must be in [1, 4]"),
                        (["--unitigs", "u", "--polish", "--realign-band", "300"], "--realign-band must be a power of two"),
                        (["--unitigs", "u", "--polish", "--realign-band", "8192"], "--realign-band must be a power of two"),
                        (["--unitigs", "u", "--polish", "--realign-min-identity", "1001"], "--realign-min-identity is in permille")):
        p = subprocess.run([_cli(), "-f", "none.txt", "-o", "none"] + flags, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and word in p.stderr.decode(), (flags, p.stderr)
