"""Graded relevance at C3 (Q=2.1k, N=190k, b=48, C=81 multi-hot, k up to 5000) and C2 (Q=10k, N=1M, b=64, C=10 one-hot): the
device route against the only route there was before hg_graded, alternating within one process.

  device   hg_graded + hg_grade_hist + hg_get_graded + hg_get_grade_hist on the lists hg_topr left (wall clock around the four
           calls, and the kernels' own HIP-event times from the timing table)
  host     hg_get_topr (Q x R x 5 bytes over PCIe) + per query a NumPy gather of the label rows, the grades and their cumulative
           sums (the sums at ks only; DCG and WAP terms would come on top)
  ideal    the Q x N label product for the ideal ordering (float32 matmul in blocks of 256 queries + a bincount per query), which
           the grade histogram replaces -- on the first `--ideal-queries` queries, scaled to Q
  topr     hg_topr itself, which both routes need

Medians of `--reps` rounds after `--warmup` rounds; one JSON line per shape (profiles/graded_timing.txt).

    python tools/graded_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases
from hashgan_amd import _native, metric
from hashgan_amd import extra_metrics as X

KS = np.array([1, 10, 100, 1000, 5000], dtype=np.int64)


def full_case(name):
    spec = dict(cases.CASES[name]); spec.pop("q_take", None)
    cases.CASES["_full"] = spec
    return cases.build_case("_full")


def med(x):
    return round(float(np.median(x)), 4)


def host_route(ctx, ql, dl):
    idx, _ = ctx.get_topr()
    out = np.empty((len(ql), len(KS)), dtype=np.int64)
    dl16, ql16 = dl.astype(np.int16), ql.astype(np.int16)
    for q in range(len(ql)):
        out[q] = np.cumsum(dl16[idx[q]] @ ql16[q], dtype=np.int64)[KS - 1]
    return out


def ideal_route(ql, dl, nq):
    dlf = np.ascontiguousarray(dl.astype(np.float32).T)
    C = ql.shape[1]
    hist = np.empty((nq, C + 1), dtype=np.int64)
    for q0 in range(0, nq, 256):
        G = (ql[q0:min(q0 + 256, nq)].astype(np.float32) @ dlf).astype(np.int16)
        for i in range(len(G)):
            hist[q0 + i] = np.bincount(G[i], minlength=C + 1)
    return hist


def run(name, label, args):
    c = full_case(name)
    qb, db, ql, dl = c["qbits"], c["dbbits"], c["qlab"], c["dblab"]
    Q, N, b, C = len(qb), len(db), c["b"], dl.shape[1]
    R = int(KS[-1])
    gain, disc = X.gain_table("exp", C), X.discount_table(R)
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), b, C)
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
    ctx.timing_enable(2)
    s = {k: [] for k in ("topr_wall", "device_wall", "graded_wall", "grade_hist_wall", "get_wall", "k_graded", "k_grade_hist",
                         "k_grade_hist_reduce", "topr_kernels", "host_wall")}
    same = None
    for rep in range(args.warmup + args.reps):
        ctx.timing_reset()
        t0 = time.perf_counter()
        ctx.topr(R)
        t1 = time.perf_counter()
        tk = sum(ms for k, (ms, n) in ctx.timing_read().items() if k != "step_gpu_span")    # (the span nests around the kernels)
        ctx.timing_reset()
        t2 = time.perf_counter()
        ctx.graded(KS, gain, disc)
        t3 = time.perf_counter()
        ctx.grade_hist()
        t4 = time.perf_counter()
        gsum = ctx.get_graded()[0]
        hist = ctx.get_grade_hist()
        t5 = time.perf_counter()
        t = ctx.timing_read()
        host = None
        if rep >= args.warmup + args.reps - args.host_reps - 1:          # (one warm-up round of its own)
            t6 = time.perf_counter()
            host = host_route(ctx, ql, dl)
            t7 = time.perf_counter()
            same = bool(np.array_equal(host, gsum))
        if rep >= args.warmup:
            s["topr_wall"].append((t1 - t0) * 1e3); s["topr_kernels"].append(tk)
            s["device_wall"].append((t5 - t2) * 1e3); s["graded_wall"].append((t3 - t2) * 1e3)
            s["grade_hist_wall"].append((t4 - t3) * 1e3); s["get_wall"].append((t5 - t4) * 1e3)
            for k in ("k_graded", "k_grade_hist", "k_grade_hist_reduce"):
                s[k].append(t[k][0] / max(1, t[k][1]))
            if host is not None and rep > args.warmup + args.reps - args.host_reps - 1:
                s["host_wall"].append((t7 - t6) * 1e3)
    nq = min(Q, args.ideal_queries)
    t0 = time.perf_counter()
    ih = ideal_route(ql, dl, nq)
    ideal_ms = (time.perf_counter() - t0) * 1e3
    out = {"case": label, "Q": Q, "N": N, "b": b, "C": C, "ks": KS.tolist(), "segments": ctx.get_stat("segments"),
           "gsum_host_equals_device": same, "grade_hist_equals_label_product": bool(np.array_equal(ih, hist.T[:nq])),
           "ms_median": {k: med(v) for k, v in s.items()}, "ms_all": {k: [round(x, 3) for x in v] for k, v in s.items()},
           "ideal_label_product_ms": {"queries": nq, "measured": round(ideal_ms, 2), "scaled_to_Q": round(ideal_ms * Q / nq, 2)},
           "list_bytes_over_pcie_host_route": Q * R * 5, "table_bytes_device_route": Q * len(KS) * 32 + Q * (C + 1) * 4}
    m = out["ms_median"]
    out["ratio"] = {"host_wall / device_wall": round(m["host_wall"] / m["device_wall"], 2),
                    "graded_wall / topr_wall": round(m["graded_wall"] / m["topr_wall"], 3),
                    "k_graded / topr_kernels": round(m["k_graded"] / m["topr_kernels"], 3)}
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--ideal-queries", type=int, default=512)
    ap.add_argument("--shapes", default="c3,c2")
    a = ap.parse_args()
    if "c3" in a.shapes:
        run("c3_nus_q64", "C3 (Q=2.1k, N=190k, b=48, C=81 multi-hot)", a)
    if "c2" in a.shapes:
        run("c2_q64", "C2 (Q=10k, N=1M, b=64, C=10 one-hot)", a)
