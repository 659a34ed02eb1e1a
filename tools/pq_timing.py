"""Quantised ranking (hg_map_pq) beside hg_map_real on the decoded float table of the same codes -- the only way to this ranking without
it -- on resident tables, at 10k x 1M x 64 (M = 8 subspaces of 8 features, K = 256: 64 KB of codebooks),
R = 5000, and at the NUS-WIDE shape of DESIGN section 8 (Q=5000, N=168 692, the same quantiser).  tanh queries; codebooks = K rows
of tanh features per subspace, codes drawn uniformly (what a timing needs of them: the decoded rows are tanh-distributed subvectors).
"c2_72" is the first shape with a ninth subspace: 72 KB of codebooks, more than the 64 KB that an LDS-staged form of k_pq_rescore
(measured and removed) could hold.

  pq         hg_map_pq (wall clock around the call), its kernels' own HIP-event times (k_pq_image16 once per database, the filter
             k_real_select, k_pq_rescore, the samples, the rank kernel), device_bytes of its context (codes, codebooks, query floats)
  real       hg_map_real on a second context that holds the decoded table (keep_floats = 1): the same, with k_real_rescore and the
             image built from floats (k_pack); in the same rounds, alternating with `pq`
  host       only with --host: from host arrays, MAPs(R, quantised=True).get_maps_by_feature against the 'reference'-mode call on the
             decoded table (fresh writable arrays each round: no residency)

Medians of `--reps` rounds after `--warmup` rounds, and each leg's min - max spread; one JSON line per shape (profiles/pq_timing.txt).

    python tools/pq_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time, types
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hashgan_amd import _native, pq, MAPs

#          label, Q, N, M, dsub, K, C, R
SHAPES = {"c2": ("10k x 1M x 64 (M=8, dsub=8, K=256, C=10, R=5000)", 10000, 1000000, 8, 8, 256, 10, 5000),
          "nus": ("NUS-WIDE shape (Q=5000, N=168692, M=8, dsub=8, K=256, C=21, R=5000)", 5000, 168692, 8, 8, 256, 21, 5000),
          "c2_72": ("10k x 1M x 72 (M=9, dsub=8, K=256: 72 KB of codebooks)", 10000, 1000000, 9, 8, 256, 10, 5000),
          "small": ("small (Q=500, N=100k, M=8, dsub=8, K=256, C=10, R=1000)", 500, 100000, 8, 8, 256, 10, 1000)}
SLOTS = {"filter": ("k_real_select", "k_real_select"), "rescore": ("k_pq_rescore", "k_real_rescore"), "sample": ("k_real_sample", "k_real_sample"),
         "guess": ("k_real_guess", "k_real_guess"), "rank": ("k_radix_pass", "k_radix_pass")}


def med(x):
    return round(float(np.median(x)), 4) if len(x) else None


def kernel_ms(t, k):
    return round(t[k][0], 4) if k in t and t[k][1] else 0.0


def run(key, args):
    label, Q, N, M, dsub, K, C, R = SHAPES[key]
    b = M * dsub
    rng = np.random.default_rng(5)
    qf = np.tanh(rng.standard_normal((Q, b), dtype=np.float32))
    books = np.tanh(rng.standard_normal((M, K, dsub), dtype=np.float32))
    codes = rng.integers(0, K, (N, M)).astype(np.uint8)
    dl = np.eye(C, dtype=np.int64)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int64)[rng.integers(0, C, Q)]
    x = pq.decode(codes, books)
    a, r = _native.Context(0), _native.Context(0)
    a.preload()                                        # (the code objects now: the first call's image build is then the kernel alone)
    a.set_option("keep_query_floats", 1)
    a.set_database_pq(codes, books, dl); a.set_queries_f32(qf, ql)
    r.set_option("keep_floats", 1)
    r.set_database_f32(x, dl); r.set_queries_f32(qf, ql)
    loaded = {"pq": a.get_stat("device_bytes"), "real": r.get_stat("device_bytes")}
    a.timing_enable(2); r.timing_enable(2)
    s = {w + "_" + k: [] for w in ("pq", "real") for k in ["wall"] + list(SLOTS)}
    first = {}
    same = None
    for rep in range(args.warmup + args.reps):
        timed = rep >= args.warmup
        res = {}
        for i, (who, ctx, call) in enumerate((("pq", a, a.map_pq), ("real", r, r.map_real))):       # alternating within the round
            ctx.timing_reset()
            t0 = time.perf_counter()
            res[who] = call(R)
            t1 = time.perf_counter()
            t = ctx.timing_read()
            if rep == 0:                                                                  # the first call builds the image
                first[who] = {"wall": round((t1 - t0) * 1e3, 4), "image": kernel_ms(t, "k_pq_image16" if who == "pq" else "k_pack")}
            if timed:
                s[who + "_wall"].append((t1 - t0) * 1e3)
                for slot, kernels in SLOTS.items():
                    s[who + "_" + slot].append(kernel_ms(t, kernels[i]))
        if rep == 0:
            same = bool(np.array_equal(res["pq"][0], res["real"][0], equal_nan=True) and np.array_equal(res["pq"][1], res["real"][1]))
    m = {k: med(v) for k, v in s.items()}
    out = {"case": label, "Q": Q, "N": N, "b": b, "M": M, "dsub": dsub, "K": K, "C": C, "R": R, "ap_and_hits_equal": same, "ms_median": m,
           "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in s.items()},
           "ms_all": {k: [round(v_, 4) for v_ in v] for k, v in s.items()}, "first_call_ms": first,
           "device_bytes_loaded": loaded,
           "device_bytes": {"pq": a.get_stat("device_bytes"), "real": r.get_stat("device_bytes")},
           "stats": {w: {k: c.get_stat(k) for k in ("real_path", "real_attempts", "real_requeried")} for w, c in (("pq", a), ("real", r))},
           "pq_float_rows": a.get_stat("pq_float_rows"),
           "ratio": {"pq_wall / real_wall": round(m["pq_wall"] / m["real_wall"], 3),
                     "pq_rescore / real_rescore": round(m["pq_rescore"] / m["real_rescore"], 3) if m["real_rescore"] else None}}
    a.close(); r.close()
    if args.host:
        hs = {"maps_quantised": [], "maps_reference_decoded": []}
        for rep in range(1 + args.host_reps):
            for who in hs:
                if who == "maps_quantised":
                    db = types.SimpleNamespace(codes=codes.copy(), codebooks=books.copy(), label=dl.copy())       # writable: loaded again every round
                    mm = MAPs(R, quantised=True)
                else:
                    db = types.SimpleNamespace(output=x.copy(), label=dl.copy())
                    mm = MAPs(R)
                q = types.SimpleNamespace(output=qf.copy(), label=ql.copy())
                t0 = time.perf_counter()
                v = mm.get_maps_by_feature(db, q)
                t1 = time.perf_counter()
                mm.close()
                if rep:
                    hs[who].append((t1 - t0) * 1e3)
                out.setdefault("host_map", {})[who] = v
        out["host_ms_median"] = {k: med(v) for k, v in hs.items()}
        out["host_ms_all"] = {k: [round(v_, 3) for v_ in v] for k, v in hs.items()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--shapes", default="c2,nus")
    a = ap.parse_args()
    for key in a.shapes.split(","):
        run(key, a)
