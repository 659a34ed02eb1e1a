"""The literal call `MAPs(R).get_maps_by_feature(database, query)` (main.py:164: a new MAPs object per evaluation) from HOST arrays
and from arrays already in DEVICE memory (devarray.DeviceArray -> hg_set_database_dev / hg_set_queries_dev), wall clock per call:

  c2_pm1      Q=10k, N=1M, b=64, C=10, R=5000   +-1 codes (planted, flip 0.30): Hamming kernels
  c2_tanh     the same shape, tanh features: float32 inner-product ranking
  cifar_tanh  Q=1k, N=54k, b=64, C=10, R=N      tanh features (config/cifar_evaluation.yaml)

Every leg -- one shape, one side -- runs in a child process of its own under `timeout`; the first child that does not exit with 0
ends the run.  A leg is `--warmup` calls, then `--calls` (>= 20) timed ones: median, min, max and the 10th / 90th percentile.  The
device legs get their memory from a second _native.Context (scratch + memcpy_htod): no torch.  `--parent-root DIR` names a checkout of
another commit (with its library built): its host legs run in the same visit, alternating with this tree's, and `--rounds` repeats
the whole sequence so that the spread between runs of the same leg is on the page.  One JSON line per leg, then a table.

Last (`--no-loads` skips it) the two loads alone at the C2 shape on tanh features, in one more child: `hg_set_database_dev` and
`hg_set_queries_dev` per call for `keep_floats` = 0 / 1 / 2, wall clock without kernel timing and again with every kernel bracketed by
HIP events (`k_pack`: total ms and launches of one pair of loads), medians of `--calls` pairs after `--warmup`.

    python tools/dev_input_timing.py [--parent-root DIR] [--out profiles/dev_input_timing.txt]      # from the repository root, on an MI355X
"""
import argparse, json, os, subprocess, sys, time, types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "c2_pm1": dict(Q=10000, N=1000000, b=64, C=10, R=5000, real=False),
    "c2_tanh": dict(Q=10000, N=1000000, b=64, C=10, R=5000, real=True),
    "cifar_tanh": dict(Q=1000, N=54000, b=64, C=10, R=54000, real=True),
}


def child(shape, side, calls, warmup, root):
    sys.path.insert(0, root)
    import numpy as np
    from hashgan_amd import MAPs, _native, synth
    s = SHAPES[shape]
    Q, N, b, C, R = s["Q"], s["N"], s["b"], s["C"], s["R"]
    dl, _ = synth.onehot_labels(1, N, C)
    ql, _ = synth.onehot_labels(2, Q, C)
    dl, ql = dl.astype(np.int64), ql.astype(np.int64)
    if s["real"]:
        rng = np.random.default_rng(0xD1)
        db, q = (np.tanh(rng.standard_normal((m, b), dtype=np.float32)) for m in (N, Q))
    else:
        db, q = (synth.planted_codes(3, lab, b, 0.30).astype(np.float32) * 2 - 1 for lab in (dl, ql))
    producer = None
    if side == "device":
        from hashgan_amd.devarray import DeviceArray
        producer = _native.Context(0)

        def dev(slot, a):
            a = np.ascontiguousarray(a)
            ptr = producer.scratch(slot, a.nbytes)
            producer.memcpy_htod(ptr, a, a.nbytes)
            return DeviceArray(ptr, a.shape, None, str(a.dtype))
        database = types.SimpleNamespace(output=dev(0, db), label=dev(1, dl))
        query = types.SimpleNamespace(output=dev(2, q), label=dev(3, ql))
    else:
        database, query = types.SimpleNamespace(output=db, label=dl), types.SimpleNamespace(output=q, label=ql)
    ms, vals = [], []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        v = MAPs(R).get_maps_by_feature(database, query)         # (complete on return: the mean needs the downloaded APs)
        t1 = time.perf_counter()
        if i >= warmup:
            ms.append((t1 - t0) * 1e3)
        vals.append(float(v))
    assert all(v == vals[0] for v in vals), vals
    ms.sort()
    pick = lambda f: round(ms[min(len(ms) - 1, int(f * len(ms)))], 3)
    print(json.dumps({"shape": shape, "side": side, "Q": Q, "N": N, "b": b, "C": C, "R": R, "calls": calls, "warmup": warmup,
                      "median_ms": round(float(np.median(ms)), 3), "min_ms": pick(0), "p10_ms": pick(0.1), "p90_ms": pick(0.9),
                      "max_ms": round(ms[-1], 3), "map": vals[0]}), flush=True)
    if producer is not None:
        producer.close()


def loads_child(calls, warmup, root):
    """The two device-array loads alone at the C2 shape: one JSON line per (keep_floats, timing level)."""
    sys.path.insert(0, root)
    import numpy as np
    from hashgan_amd import _native
    from hashgan_amd.devarray import DeviceArray
    s = SHAPES["c2_tanh"]
    Q, N, b, C = s["Q"], s["N"], s["b"], s["C"]
    rng = np.random.default_rng(0xD1)
    db, q = (np.tanh(rng.standard_normal((m, b), dtype=np.float32)) for m in (N, Q))
    eye = np.eye(C, dtype=np.int64)
    dl, ql = eye[rng.integers(0, C, N)], eye[rng.integers(0, C, Q)]
    producer, ctx = _native.Context(0), _native.Context(0)

    def dev(slot, a):
        ptr = producer.scratch(slot, a.nbytes)
        producer.memcpy_htod(ptr, a, a.nbytes)
        return DeviceArray(ptr, a.shape, None, str(a.dtype))
    fd, ld, fq, lq = dev(0, db), dev(1, dl), dev(2, q), dev(3, ql)
    for keep in (0, 1, 2):
        ctx.set_option("keep_floats", keep)
        for level in (0, 2):
            ctx.timing_enable(level)
            t_db, t_q = [], []
            for i in range(warmup + calls):
                ctx.timing_reset()
                t0 = time.perf_counter()
                ctx.set_database_dev(fd, ld)
                t1 = time.perf_counter()
                ctx.set_queries_dev(fq, lq)
                t2 = time.perf_counter()
                if i >= warmup:
                    t_db.append((t1 - t0) * 1e3)
                    t_q.append((t2 - t1) * 1e3)
            kp = ctx.timing_read().get("k_pack")
            print(json.dumps({"loads": "c2_tanh", "Q": Q, "N": N, "b": b, "C": C, "keep_floats": keep, "kernel_timing": level, "calls": calls,
                              "set_database_dev_ms": round(float(np.median(t_db)), 4), "set_queries_dev_ms": round(float(np.median(t_q)), 4),
                              "k_pack_ms_of_one_pair": round(kp[0], 4) if kp else None, "k_pack_launches": kp[1] if kp else None,
                              "bytes_read_by_the_packs": int(db.nbytes + dl.nbytes + q.nbytes + ql.nbytes + (db.nbytes if keep == 2 else 0))}),
                  flush=True)                                    # (keep_floats = 2 on tanh features: the database's floats in a second pass)
    ctx.close()
    producer.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=24)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--shapes", default="c2_pm1,c2_tanh,cifar_tanh")
    p.add_argument("--parent-root", default=None, help="a checkout of another commit, library built: its host legs run beside this tree's")
    p.add_argument("--limit", type=int, default=240, help="seconds a leg may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dev_input_timing.txt"))
    p.add_argument("--no-loads", action="store_true", help="skip the leg that times the two loads alone")
    p.add_argument("--child", nargs=3, metavar=("SHAPE", "SIDE", "ROOT"), default=None)
    a = p.parse_args()
    if a.child and a.child[0] == "loads":
        return loads_child(a.calls, a.warmup, a.child[2])
    if a.child:
        return child(a.child[0], a.child[1], a.calls, a.warmup, a.child[2])
    if a.calls < 20:
        p.error("--calls must be >= 20")
    legs = ([("parent", "host", os.path.abspath(a.parent_root))] if a.parent_root else []) + [("this", "host", ROOT), ("this", "device", ROOT)]
    lines, rows = [], []
    for rnd in range(a.rounds):
        for shape in a.shapes.split(","):
            for tree, side, root in legs:
                env = dict(os.environ)
                env.pop("HG_LIBRARY", None)
                r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--calls", str(a.calls),
                                    "--warmup", str(a.warmup), "--child", shape, side, root], capture_output=True, text=True, env=env)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    sys.exit("leg %s / %s / %s of round %d ended with status %d: stopping" % (shape, tree, side, rnd, r.returncode))
                rec = json.loads(r.stdout.strip().splitlines()[-1])
                rec.update(tree=tree, round=rnd)
                rows.append(rec)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    lines.append("")
    lines.append("%-11s %-7s %-7s %s" % ("shape", "tree", "side", "median ms per round (min .. max of the round's calls)"))
    for shape in a.shapes.split(","):
        for tree, side, _ in legs:
            mine = [r for r in rows if (r["shape"], r["tree"], r["side"]) == (shape, tree, side)]
            lines.append("%-11s %-7s %-7s %s" % (shape, tree, side, "   ".join("%.3f (%.3f .. %.3f)" % (r["median_ms"], r["min_ms"], r["max_ms"]) for r in mine)))
        maps = {r["map"] for r in rows if r["shape"] == shape}
        lines.append("%-11s mAP identical on every leg: %s" % (shape, len(maps) == 1))
    if not a.no_loads:
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--calls", str(a.calls),
                            "--warmup", str(a.warmup), "--child", "loads", "device", ROOT], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("the loads leg ended with status %d: stopping" % r.returncode)
        lines += ["", "the two loads alone (C2 shape, tanh features), median ms per call:"] + [l for l in r.stdout.splitlines() if l.startswith("{")]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
