#!/usr/bin/env python3
"""The identity threshold of the clipped ends, measured on the CPU with the test kit's mirrors alone: no device.

Per trial: a random template of --template bases, two copies at --error (bella_testkit.trace_cases._noisy), --junk random bases
appended to both; the extension of bella_testkit.trace_mirror.banded_extension on --band diagonals from (0, 0); then the clip of
bella_testkit.clip_mirror at every --identity.  Recorded per identity: the distance of the clip's end on V to the true boundary
with junk, the bases a clip takes from the pairs without junk, and the identity per column of the homologous part and of the junk.
Writes profiles/clip_probe.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bella_testkit import clip_mirror as K          # noqa: E402
from bella_testkit import trace_cases as TC         # noqa: E402
from bella_testkit import trace_mirror as M         # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--trials", type=int, default=40)
    ap.add_argument("--template", type=int, default=2000)
    ap.add_argument("--junk", type=int, default=1500)
    ap.add_argument("--error", type=float, default=0.15)
    ap.add_argument("--band", type=int, default=1024)
    ap.add_argument("--identity", type=int, nargs="+", default=[550, 600, 650, 700, 750])
    ap.add_argument("--seed", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_probe.json"))
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ext_end, id_hom, id_junk = [], [], []
    dist = {t: [] for t in a.identity}
    lost = {t: [] for t in a.identity}
    kept_junk = {t: [] for t in a.identity}
    for _ in range(a.trials):
        tmpl = TC._rand(rng, a.template)
        v0, h0 = TC._noisy(rng, tmpl, a.error), TC._noisy(rng, tmpl, a.error)
        for junk in (True, False):
            v, h = (v0 + TC._rand(rng, a.junk), h0 + TC._rand(rng, a.junk)) if junk else (v0, h0)
            _, (bi, bj), steps, _ = M.banded_extension(h, v, a.band)
            ops = np.asarray(steps[::-1], np.int64)                         # from (0, 0) outwards
            words = M.run_lengths(ops)
            if junk:
                # the columns of the homologous part: those that begin before either copy ends
                i = np.concatenate([[0], np.cumsum(ops != K.DEL)])[:-1]
                j = np.concatenate([[0], np.cumsum(ops != K.INS)])[:-1]
                hom = (i < len(v0)) & (j < len(h0))
                ext_end.append(int(len(v) - bi))
                id_hom.append(float((ops[hom] == K.EQ).mean()))
                if (~hom).sum() > 100:
                    id_junk.append(float((ops[~hom] == K.EQ).mean()))
            for t in a.identity:
                r = K.clip_one(words, 0, 0, t)
                if junk:
                    dist[t].append(abs(int(r["endV"]) - len(v0)))
                    kept_junk[t].append(max(0, int(r["endV"]) - len(v0)))
                else:
                    lost[t].append((bi - (int(r["endV"]) - int(r["begV"]))) + (bj - (int(r["endH"]) - int(r["begH"]))))
    q = lambda x: dict(min=float(np.min(x)), median=float(np.median(x)), p90=float(np.percentile(x, 90)), max=float(np.max(x)), mean=float(np.mean(x)))
    out = dict(machine="CPU only: the numpy mirrors, no device", trials=a.trials, template=a.template, junk=a.junk, error=a.error, band=a.band, seed=a.seed,
               extension_end_to_end_of_junk=q(ext_end), identity_per_column_homologous=q(id_hom), identity_per_column_junk=q(id_junk),
               per_identity={str(t): dict(distance_to_true_boundary_with_junk=q(dist[t]), junk_bases_kept=q(kept_junk[t]),
                                          bases_lost_without_junk_both_reads=q(lost[t])) for t in a.identity})
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
