"""hg_map_rerank beside hg_map_real and hg_map of the same build, in one process per shape on resident tables (keep_floats = 1):

  c2     Q=10k, N=1M, b=64, C=10, R=5000    tanh of planted codes (flip 0.30) plus noise
  cifar  Q=1k, N=54k, b=64, C=10, R=N       the same generator (config/cifar_evaluation.yaml's shape)

Per shape a child process under `timeout` (the first that does not exit with 0 ends the run): `--warmup` calls of each entry point, then
`--calls` timed ones (wall clock of the whole call, download included: median, min, max), then one call of each with every kernel
bracketed by HIP events -- the per-kernel split from hg_timing_read -- and the re-rank's stats.  One JSON line per shape, then a table.

    python tools/rerank_timing.py [--out profiles/rerank_timing.txt]      # from the repository root, on an MI355X
"""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "c2": dict(Q=10000, N=1000000, b=64, C=10, R=5000),
    "cifar": dict(Q=1000, N=54000, b=64, C=10, R=54000),
}


def child(shape, calls, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    from hashgan_amd import _native, synth
    s = SHAPES[shape]
    Q, N, b, C, R = s["Q"], s["N"], s["b"], s["C"], s["R"]
    dl, _ = synth.onehot_labels(1, N, C)
    ql, _ = synth.onehot_labels(2, Q, C)
    dl, ql = dl.astype(np.int64), ql.astype(np.int64)
    rng = np.random.default_rng(0xD1)
    db, q = (np.tanh((synth.planted_codes(3, lab, b, 0.30).astype(np.float32) * 2 - 1) + 0.7 * rng.standard_normal((len(lab), b), dtype=np.float32))
             for lab in (dl, ql))
    ctx = _native.Context(0)
    ctx.set_option("keep_floats", 1)
    ctx.set_database_f32(db, dl)
    ctx.set_queries_f32(q, ql)
    legs = (("map_rerank", ctx.map_rerank), ("map_real", ctx.map_real), ("map", ctx.map))
    rec = {"shape": shape, "Q": Q, "N": N, "b": b, "C": C, "R": R, "calls": calls, "warmup": warmup}
    for name, fn in legs:
        ms = []
        for i in range(warmup + calls):
            t0 = time.perf_counter()
            ap, rel = fn(R)
            t1 = time.perf_counter()
            if i >= warmup:
                ms.append((t1 - t0) * 1e3)
        rec[name] = {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
                     "map": float(np.mean(ap[rel != 0]))}
    ctx.timing_enable(2)
    for name, fn in legs:
        ctx.timing_reset()
        fn(R)
        rec[name]["kernels_ms"] = {k: round(v[0], 4) for k, v in sorted(ctx.timing_read().items()) if v[1]}
        if name == "map_rerank":
            rec[name]["stats"] = {k: ctx.get_stat(k) for k in ("rerank_records", "rerank_chunks", "rerank_groups_lds", "rerank_groups_global", "segments")}
    ctx.close()
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=7)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--shapes", default="c2,cifar")
    p.add_argument("--limit", type=int, default=400, help="seconds a shape may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_timing.txt"))
    p.add_argument("--child", default=None)
    a = p.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup)
    lines, rows = [], []
    for shape in a.shapes.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--calls", str(a.calls),
                            "--warmup", str(a.warmup), "--child", shape], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("shape %s ended with status %d: stopping" % (shape, r.returncode))
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        lines.append(json.dumps(rows[-1]))
        print(lines[-1], flush=True)
    lines.append("")
    lines.append("%-6s %-11s %s" % ("shape", "call", "median ms (min .. max), whole call on resident tables"))
    for r in rows:
        for name in ("map_rerank", "map_real", "map"):
            t = r[name]
            lines.append("%-6s %-11s %.3f (%.3f .. %.3f)   mAP %.6f" % (r["shape"], name, t["median_ms"], t["min_ms"], t["max_ms"], t["map"]))
        lines.append("%-6s map_rerank kernels (ms, one call): %s" % (r["shape"], "  ".join("%s %.3f" % kv for kv in r["map_rerank"]["kernels_ms"].items())))
        lines.append("%-6s map_rerank stats: %s" % (r["shape"], r["map_rerank"]["stats"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
