"""Asymmetric ranking (hg_map_asym) beside hg_map_real on the +-1.0 float table of the same codes -- the only way to this ranking
without it -- on resident tables, at C2 (Q=10k, N=1M, b=64, C=10, R=5000) and at the NUS-WIDE shape of DESIGN section 8
(Q=5000, N=168 692, b=64, C=21, R=5000).  tanh queries, a signed tanh database.

  asym       hg_map_asym (wall clock around the call), its kernels' own HIP-event times (k_asym_image16 once per database, the filter
             k_real_select, k_asym_rescore), device_bytes of its context (codes + query floats)
  real       hg_map_real on a second context that holds where(code bit, +1, -1) as floats (keep_floats = 1): the same, with
             k_real_rescore and the image built from floats (k_pack); in the same rounds, alternating with `asym`
  host       only with --host: from host arrays, MAPs(R, asymmetric=True).get_maps_by_feature against the 'reference'-mode call, which
             uploads the float table a second time (fresh writable arrays each round: no residency)

Medians of `--reps` rounds after `--warmup` rounds; one JSON line per shape (profiles/asym_timing.txt).

    python tools/asym_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time, types
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hashgan_amd import _native, MAPs

SHAPES = {"c2": ("C2 (Q=10k, N=1M, b=64, C=10, R=5000)", 10000, 1000000, 64, 10, 5000),
          "nus": ("NUS-WIDE shape (Q=5000, N=168692, b=64, C=21, R=5000)", 5000, 168692, 64, 21, 5000),
          "small": ("small (Q=500, N=100k, b=64, C=10, R=1000)", 500, 100000, 64, 10, 1000)}


def med(x):
    return round(float(np.median(x)), 4) if len(x) else None


def kernel_ms(t, k):
    return round(t[k][0], 4) if k in t and t[k][1] else 0.0


def run(key, args):
    label, Q, N, b, C, R = SHAPES[key]
    rng = np.random.default_rng(5)
    dbf = np.tanh(rng.standard_normal((N, b), dtype=np.float32))
    qf = np.tanh(rng.standard_normal((Q, b), dtype=np.float32))
    dl = np.eye(C, dtype=np.int64)[rng.integers(0, C, N)]
    ql = np.eye(C, dtype=np.int64)[rng.integers(0, C, Q)]
    pm1 = np.where(dbf > 0, 1, -1).astype(np.float32)
    a, r = _native.Context(0), _native.Context(0)
    a.preload()                                        # (the code objects now: the first call's image build is then the kernel alone)
    a.set_option("keep_floats", 0); a.set_option("keep_query_floats", 1)
    a.set_database_f32(dbf, dl); a.set_queries_f32(qf, ql)
    r.set_option("keep_floats", 1)
    r.set_database_f32(pm1, dl); r.set_queries_f32(qf, ql)
    a.timing_enable(2); r.timing_enable(2)
    names = ["asym_wall", "real_wall", "asym_filter", "asym_rescore", "real_filter", "real_rescore", "asym_sample", "real_sample", "asym_rank", "real_rank"]
    s = {k: [] for k in names}
    first = {}
    same = None
    for rep in range(args.warmup + args.reps):
        timed = rep >= args.warmup
        res = {}
        for who, ctx, call in (("asym", a, a.map_asym), ("real", r, r.map_real)):       # alternating within the round
            ctx.timing_reset()
            t0 = time.perf_counter()
            res[who] = call(R)
            t1 = time.perf_counter()
            t = ctx.timing_read()
            if rep == 0:                                                                  # the first call builds the image
                first[who] = {"wall": round((t1 - t0) * 1e3, 4), "image": kernel_ms(t, "k_asym_image16" if who == "asym" else "k_pack")}
            if timed:
                s[who + "_wall"].append((t1 - t0) * 1e3)
                s[who + "_filter"].append(kernel_ms(t, "k_real_select"))
                s[who + "_rescore"].append(kernel_ms(t, "k_asym_rescore" if who == "asym" else "k_real_rescore"))
                s[who + "_sample"].append(kernel_ms(t, "k_real_sample"))
                s[who + "_rank"].append(kernel_ms(t, "k_radix_pass"))
        if rep == 0:
            same = bool(np.array_equal(res["asym"][0], res["real"][0], equal_nan=True) and np.array_equal(res["asym"][1], res["real"][1]))
    m = {k: med(v) for k, v in s.items()}
    out = {"case": label, "Q": Q, "N": N, "b": b, "C": C, "R": R, "ap_and_hits_equal": same, "ms_median": m,
           "ms_all": {k: [round(x, 4) for x in v] for k, v in s.items()}, "first_call_ms": first,
           "device_bytes": {"asym": a.get_stat("device_bytes"), "real": r.get_stat("device_bytes")},
           "stats": {w: {k: c.get_stat(k) for k in ("real_path", "real_attempts", "real_requeried")} for w, c in (("asym", a), ("real", r))},
           "asym_float_rows": a.get_stat("asym_float_rows"),
           "ratio": {"asym_wall / real_wall": round(m["asym_wall"] / m["real_wall"], 3),
                     "asym_rescore / real_rescore": round(m["asym_rescore"] / m["real_rescore"], 3) if m["real_rescore"] else None}}
    a.close(); r.close()
    if args.host:
        hs = {"maps_asymmetric": [], "maps_reference_pm1": []}
        for rep in range(1 + args.host_reps):
            for who, kw, table in (("maps_asymmetric", dict(asymmetric=True), dbf), ("maps_reference_pm1", dict(), pm1)):
                db = types.SimpleNamespace(output=table.copy(), label=dl.copy())       # writable: loaded again every round
                q = types.SimpleNamespace(output=qf.copy(), label=ql.copy())
                mm = MAPs(R, **kw)
                t0 = time.perf_counter()
                v = mm.get_maps_by_feature(db, q)
                t1 = time.perf_counter()
                mm.close()
                if rep:
                    hs[who].append((t1 - t0) * 1e3)
                out.setdefault("host_map", {})[who] = v
        out["host_ms_median"] = {k: med(v) for k, v in hs.items()}
        out["host_ms_all"] = {k: [round(x, 3) for x in v] for k, v in hs.items()}
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
