"""Tie-aware AP (hg_tie_ap) on resident tables at C2 (Q=10k, N=1M, b=64, R=5000), C3 (Q=2.1k, N=190k, b=48, R=5000) and
C1 (Q=1k, N=54k, b=32, R=N=54000), alternating within one process:

  tie_ap_warm    hg_tie_ap with the relevant-row histogram of the loaded tables already there: k_tie_ap alone (wall clock around the
                 call, and the kernel's own HIP-event time from the timing table)
  tie_ap_cold    hg_tie_ap after the queries were handed over again (the tables are stale): the histogram pass (k_hist_rel, k_hist_rel_reduce) and k_tie_ap
  map            hg_map at the same R on the same tables, for comparison (wall clock, and the sum of its kernels)

Medians of `--reps` rounds after `--warmup` rounds; one JSON line per shape (profiles/tie_ap_timing.txt).  Also printed: how far
the index-order AP of hg_map lies from the expectation and how wide the envelope is, over the queries.

    python tools/tie_ap_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases
from hashgan_amd import _native, metric


def full_case(name):
    spec = dict(cases.CASES[name]); spec.pop("q_take", None)
    cases.CASES["_full"] = spec
    return cases.build_case("_full")


def med(x):
    return round(float(np.median(x)), 4)


def per_launch(t, k):
    return t[k][0] / max(1, t[k][1]) if k in t else 0.0


def run(name, label, args):
    c = full_case(name)
    qb, db, ql, dl = c["qbits"], c["dbbits"], c["qlab"], c["dblab"]
    Q, N, b, C, R = len(qb), len(db), c["b"], dl.shape[1], int(c["R"])
    Rs = np.array([R], dtype=np.int64)
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), b, C)
    qc, qw = metric.pack_codes(qb), metric.pack_labels(ql)
    ctx.set_queries(qc, qw)
    ctx.timing_enable(2)
    keys = ("tie_ap_warm_wall", "k_tie_ap", "tie_ap_cold_wall", "k_hist_rel", "k_hist_rel_reduce", "k_tie_ap_cold", "map_wall", "map_kernels")
    s = {k: [] for k in keys}
    for rep in range(args.warmup + args.reps):
        ctx.set_queries(qc, qw)
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        ctx.tie_ap(Rs)                                 # cold: no tables
        t1 = time.perf_counter()
        cold = ctx.timing_read()
        ctx.timing_reset()
        t2 = time.perf_counter()
        ctx.tie_ap(Rs)                                 # warm: the tables are there
        t3 = time.perf_counter()
        warm = ctx.timing_read()
        assert "k_hist_rel" not in warm or warm["k_hist_rel"][1] == 0
        tie = ctx.get_tie_ap()
        ctx.timing_reset()
        t4 = time.perf_counter()
        ap, rel = ctx.map(R)
        t5 = time.perf_counter()
        mk = sum(ms for k, (ms, n) in ctx.timing_read().items() if k != "step_gpu_span")     # (the span nests around the kernels)
        if rep >= args.warmup:
            s["tie_ap_cold_wall"].append((t1 - t0) * 1e3); s["tie_ap_warm_wall"].append((t3 - t2) * 1e3)
            s["map_wall"].append((t5 - t4) * 1e3); s["map_kernels"].append(mk)
            s["k_tie_ap"].append(per_launch(warm, "k_tie_ap")); s["k_tie_ap_cold"].append(per_launch(cold, "k_tie_ap"))
            s["k_hist_rel"].append(per_launch(cold, "k_hist_rel")); s["k_hist_rel_reduce"].append(per_launch(cold, "k_hist_rel_reduce"))
    hit = rel > 0
    inside = bool(((ap[hit] >= tie["ap_min"][hit, 0] * (1 - 1e-10)) & (ap[hit] <= tie["ap_max"][hit, 0] * (1 + 1e-10))).all()
                  and (rel >= tie["rel_lo"][:, 0]).all() and (rel <= tie["rel_hi"][:, 0]).all())
    w = tie["p_hit"][:, 0]
    out = {"case": label, "Q": Q, "N": N, "b": b, "C": C, "R": R, "segments": ctx.get_stat("segments"),
           "ms_median": {k: med(v) for k, v in s.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in s.items()},
           "hg_map_inside_envelope": inside,
           "map_index_order": float(np.mean(ap[hit])), "map_tie_aware": float(np.where(w > 0, w * tie["ap"][:, 0], 0.0).sum() / w.sum()),
           "mean_ap_min": float(np.nanmean(tie["ap_min"][:, 0])), "mean_ap_max": float(np.nanmean(tie["ap_max"][:, 0])),
           "largest_abs_ap_minus_expectation": float(np.nanmax(np.abs(ap - tie["ap"][:, 0]))),
           "queries_with_0_lt_p_hit_lt_1": int(((w > 0) & (w < 1)).sum())}
    m = out["ms_median"]
    out["ratio"] = {"k_tie_ap / (k_hist_rel + reduce)": round(m["k_tie_ap"] / max(m["k_hist_rel"] + m["k_hist_rel_reduce"], 1e-9), 3),
                    "tie_ap_cold_wall / map_wall": round(m["tie_ap_cold_wall"] / m["map_wall"], 3)}
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--shapes", default="c2,c3,c1")
    a = p.parse_args()
    if "c2" in a.shapes:
        run("c2_q64", "C2 (Q=10k, N=1M, b=64, C=10 one-hot, R=5000)", a)
    if "c3" in a.shapes:
        run("c3_nus_q64", "C3 (Q=2.1k, N=190k, b=48, C=81 multi-hot, R=5000)", a)
    if "c1" in a.shapes:
        run("c1_cifar_full", "C1 (Q=1k, N=54k, b=32, C=10, R=N=54000)", a)
