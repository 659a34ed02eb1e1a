"""The exact PQ encoder on the GPU (hg_pq_encode / hg_pq_encode_dev, k_pq_encode) beside pq.encode on the same machine's host, at
1M x 64 (M = 8 subspaces of 8 features, K = 256) and at the NUS-WIDE shape of DESIGN section 8 (N = 168 692, the same quantiser);
"b255" (N = 200 000, M = 5, dsub = 51) is the generic path.  tanh features; codebooks = K rows of the features per subspace.

  kernel     k_pq_encode's own time by HIP events (the context's kernel timing), summed over the call's chunks
  host_call  hg_pq_encode from host arrays: wall clock around the call -- upload in chunks, kernel, codes back
  dev_call   hg_pq_encode_dev on the same features in device memory: wall clock around the call -- kernel, codes back
  pq_encode  pq.encode (NumPy, float64) on the first `--host-rows` rows, once, and that time scaled by N / rows: an extrapolation
  floor      the float64 vector-issue floor: 3 N M K dsub lane-operations (subtract, multiply, add) over the chip's float64 vector rate,
             256 CUs x 4 SIMDs x 16 lanes per clock x 2.4 GHz = 39.3e12 lane-operations per second.  (MI355X_MICROARCH's chip parameters
             give the float32 vector peak as 157.3 TFLOPS = 256 x 4 x 32 lanes x 2 x 2.4 GHz; the float64 vector peak of the data sheet
             is half of it, 78.6 TFLOPS, hence 16 lanes per clock.)  Derived, not measured; `kernel_over_floor` = kernel / floor.

Medians of `--reps` rounds after `--warmup` rounds, host and device calls alternating within a round, and each leg's min - max;
one JSON line per shape (profiles/pq_encode_timing.txt).  The codes of both calls are compared with each other and, on the slice, with
pq.encode's.

    python tools/pq_encode_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hashgan_amd import _native, pq
from hashgan_amd.devarray import DeviceArray

#          label, N, M, dsub, K
SHAPES = {"c2": ("1M x 64 (M=8, dsub=8, K=256)", 1000000, 8, 8, 256),
          "nus": ("NUS-WIDE shape (N=168692, M=8, dsub=8, K=256)", 168692, 8, 8, 256),
          "b255": ("200k x 255 (M=5, dsub=51, K=256): the generic path", 200000, 5, 51, 256),
          "small": ("small (N=20000, M=8, dsub=8, K=256)", 20000, 8, 8, 256)}
F64_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9


def run(key, args):
    label, N, M, dsub, K = SHAPES[key]
    b = M * dsub
    rng = np.random.default_rng(5)
    x = np.tanh(rng.standard_normal((N, b), dtype=np.float32))
    books = np.stack([x[rng.choice(N, K, replace=False), m * dsub:(m + 1) * dsub] for m in range(M)])
    ctx, prod = _native.Context(0), _native.Context(0)
    ctx.preload()
    ptr = prod.scratch(0, x.nbytes)
    prod.memcpy_htod(ptr, x, x.nbytes)
    dev = DeviceArray(ptr, x.shape)
    ctx.timing_enable(2)
    s = {k: [] for k in ("host_call", "host_kernel", "dev_call", "dev_kernel")}
    codes, launches = {}, {}
    for rep in range(args.warmup + args.reps):
        for who, src in (("host", x), ("dev", dev)):                  # alternating within the round
            ctx.timing_reset()
            t0 = time.perf_counter()
            c, _, bad = ctx.pq_encode(src, books)                     # (complete on return: the call synchronises)
            t1 = time.perf_counter()
            t = ctx.timing_read()
            assert bad == 0
            codes[who] = c
            launches[who] = t["k_pq_encode"][1]
            if rep >= args.warmup:
                s[who + "_call"].append((t1 - t0) * 1e3)
                s[who + "_kernel"].append(t["k_pq_encode"][0])
    rows = min(args.host_rows, N)
    t0 = time.perf_counter()
    ref = pq.encode(x[:rows], books)
    host_ms = (time.perf_counter() - t0) * 1e3
    med = {k: round(float(np.median(v)), 4) for k, v in s.items()}
    floor_ms = 3.0 * N * M * K * dsub / F64_LANE_OPS_PER_S * 1e3
    out = {"case": label, "N": N, "b": b, "M": M, "dsub": dsub, "K": K,
           "codes_equal": {"host_call == dev_call": bool(np.array_equal(codes["host"], codes["dev"])),
                           "== pq.encode on the slice": bool(np.array_equal(codes["dev"][:rows], ref))},
           "ms_median": med, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in s.items()},
           "ms_all": {k: [round(v_, 4) for v_ in v] for k, v in s.items()},
           "f64_floor": {"lane_ops": 3 * N * M * K * dsub, "lane_ops_per_s": F64_LANE_OPS_PER_S, "floor_ms": round(floor_ms, 4),
                         "kernel_over_floor": round(med["dev_kernel"] / floor_ms, 3), "fraction_of_floor_rate": round(floor_ms / med["dev_kernel"], 3)},
           "pq_encode_host": {"rows": rows, "ms": round(host_ms, 1), "extrapolated_to_N_ms": round(host_ms * N / rows, 1),
                              "extrapolated / dev_call": round(host_ms * N / rows / med["dev_call"], 1),
                              "extrapolated / host_call": round(host_ms * N / rows / med["host_call"], 1)},
           "launches_per_call": {"host": launches["host"], "dev": launches["dev"]}, "device_bytes": ctx.get_stat("device_bytes")}
    ctx.close(); prod.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=100000)
    ap.add_argument("--shapes", default="c2,nus,b255")
    a = ap.parse_args()
    for key in a.shapes.split(","):
        run(key, a)
