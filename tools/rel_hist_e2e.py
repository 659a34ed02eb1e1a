"""End to end: extra_metrics.precision_within_radius(radius=2) at C2 (Q = 10k, N = 1M, b = 64) and precision_recall_at_k at
Q = 1000, N = 100k, timed call by call on the package under ROOT -- this tree, or an export of another commit with its own library
built (git archive <commit> hashgan_amd include | tar -x -C DIR; python -m hashgan_amd.build there) -- and dumped to OUT/e2e_TAG.npz
for comparison.  One JSON line.

    python tools/rel_hist_e2e.py TAG ROOT [OUT]
"""
import json, os, sys, time
import numpy as np
which, root = sys.argv[1], sys.argv[2]
outdir = sys.argv[3] if len(sys.argv) > 3 else "."
sys.path.insert(0, os.path.abspath(root))
import hashgan_amd
assert os.path.abspath(hashgan_amd.__file__).startswith(os.path.abspath(root)), hashgan_amd.__file__
from hashgan_amd import extra_metrics as X, synth


def planted(seed, Q, N, b, C, flip):
    dblab, _ = synth.onehot_labels(seed * 3 + 1, N, C)
    qlab, _ = synth.onehot_labels(seed * 3 + 2, Q, C)
    dbbits = synth.planted_codes(seed, dblab, b, flip)
    qbits = synth.planted_codes(seed, qlab, b, flip) ^ (synth.random_bits(seed + 17, Q, b) & synth.random_bits(seed + 18, Q, b))
    return qbits, dbbits, qlab, dblab


out = {"which": which}
qb, db, ql, dl = planted(0xC2, 10000, 1000000, 64, 10, 0.30)
ts = []
for rep in range(4):
    t0 = time.perf_counter()
    prec, ball = X.precision_within_radius(qb, db, ql, dl, radius=2)
    ts.append((time.perf_counter() - t0) * 1e3)
out["pwr_c2_ms"] = [round(t, 2) for t in ts]
out["pwr_c2_ball_max"] = int(ball.max())
out["pwr_c2_prec"] = repr(prec)
np.savez(os.path.join(outdir, "e2e_%s.npz" % which), ball=ball, prec=np.float64(prec))
qb, db, ql, dl = planted(0xC9, 1000, 100000, 64, 10, 0.30)
ks = [1, 10, 100, 1000]
ts = []
for rep in range(3):
    t0 = time.perf_counter()
    p, r = X.precision_recall_at_k(qb, db, ql, dl, ks)
    ts.append((time.perf_counter() - t0) * 1e3)
out["prk_1000x100k_ms"] = [round(t, 2) for t in ts]
prec4, ball4 = X.precision_within_radius(qb, db, ql, dl, radius=24)      # a radius with crowded balls, at the smaller size
out["pwr_1000x100k_r24_ball_max"] = int(ball4.max())
z = dict(np.load(os.path.join(outdir, "e2e_%s.npz" % which)))
np.savez(os.path.join(outdir, "e2e_%s.npz" % which), p=p, r=r, ball4=ball4, prec4=np.float64(prec4), **z)
print(json.dumps(out), flush=True)
