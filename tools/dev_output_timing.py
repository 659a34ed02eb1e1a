"""Ranked lists and match bits into resident DEVICE buffers (hg_export) against the host route over the same results, on one context:

  c2   Q=10k,  N=1M,   b=64, C=10, R=5000   +-1 codes (planted, flip 0.30)
  c3   Q=2100, N=190k, b=48, C=81, R=5000   +-1 codes, multi-hot labels

  leg A  one hg_export of IDX (int64) + DIST (uint8) + MATCH (uint8) into resident buffers, wall clock, complete on return
  leg B  the host route: get_topr + get_match (the downloads, the bitmap expanded on the CPU), wall clock
  leg C  k_export alone per item from the timing slots (HIP events around the launch): bytes read + written over its time, beside the
         rate a float4 copy reaches on this part (6.29 TB/s measured; 8 TB/s on paper)

Medians of `--rounds` (5) timed rounds after `--warmup` (3), with the smallest and the largest round beside them.  Each shape runs in a
child process of its own under `timeout`; the first child that does not exit with 0 ends the run.  The device buffers come from a second
_native.Context (scratch): no torch.  After the timed rounds the exported buffers are read back once and compared with the getters.

    python tools/dev_output_timing.py [--out profiles/dev_output_timing.txt]      # from the repository root, on an MI355X
"""
import argparse, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "c2": dict(Q=10000, N=1000000, b=64, C=10, R=5000, multihot=False),
    "c3": dict(Q=2100, N=190000, b=48, C=81, R=5000, multihot=True),
}
COPY_RATE_TBS = 6.29       # float4 copy, measured on the MI355X (8.0 on paper)


def child(shape, rounds, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    from hashgan_amd import _native, synth
    from hashgan_amd.devarray import DeviceOut
    s = SHAPES[shape]
    Q, N, b, C, R = s["Q"], s["N"], s["b"], s["C"], s["R"]
    rng = np.random.default_rng(0xD0)
    if s["multihot"]:
        dl, ql = ((rng.random((m, C)) < 0.05).astype(np.int64) for m in (N, Q))
        db, q = (np.where(rng.random((m, b)) < 0.5, 1.0, -1.0).astype(np.float32) for m in (N, Q))
    else:
        dl, _ = synth.onehot_labels(1, N, C)
        ql, _ = synth.onehot_labels(2, Q, C)
        dl, ql = dl.astype(np.int64), ql.astype(np.int64)
        db, q = (synth.planted_codes(3, lab, b, 0.30).astype(np.float32) * 2 - 1 for lab in (dl, ql))
    ctx, producer = _native.Context(0), _native.Context(0)
    ctx.set_database_f32(db, dl)
    ctx.set_queries_f32(q, ql)
    ctx.topr(R)
    ctx.match()
    RW = (R + 63) // 64
    items = {"idx": ("int64", 8, Q * R * (4 + 8)), "dist": ("uint8", 1, Q * R * 2), "match": ("uint8", 1, Q * RW * 8 + Q * R)}
    dst = {n: DeviceOut(producer.scratch(i, Q * R * isz), (Q, R), None, dt) for i, (n, (dt, isz, _)) in enumerate(items.items())}
    call = [(n, dst[n]) for n in items]
    # byte rows of R = 5000 are no multiple of 16 bytes: contiguous uint8 destinations go element-wise.  The same two items once more
    # into rows pitched to a multiple of 16 (the 16-byte store path), for leg C
    pitch = (R + 15) // 16 * 16
    wide = producer.scratch(3, 2 * Q * pitch)
    pitched = {"dist": DeviceOut(wide, (Q, R), (pitch, 1), "uint8"), "match": DeviceOut(wide + Q * pitch, (Q, R), (pitch, 1), "uint8")}

    def timed(fn):
        ms = []
        for i in range(warmup + rounds):
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    def host_route():
        ctx.get_topr()
        ctx.get_match()

    stats = lambda ms: {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    out = {"shape": shape, "Q": Q, "N": N, "b": b, "C": C, "R": R, "rounds": rounds, "warmup": warmup}
    out["A_export_idx64_dist_match"] = stats(timed(lambda: ctx.export(call)))
    out["A_export_variant"] = ctx.get_stat("export_variant")
    out["A_export_bytes"] = ctx.get_stat("export_bytes")
    out["B_host_get_topr_get_match"] = stats(timed(host_route))
    ctx.timing_enable(2)
    for n, (dt, isz, traffic) in items.items():
        ms = []
        for i in range(warmup + rounds):
            ctx.timing_reset()
            ctx.export([(n, dst[n])])
            t = ctx.timing_read()["k_export"]
            assert t[1] == 1
            if i >= warmup:
                ms.append(t[0])
        st = stats(ms)
        st.update(bytes_read_and_written=traffic, tb_per_s=round(traffic / (st["median_ms"] * 1e-3) / 1e12, 3),
                  share_of_copy_rate=round(traffic / (st["median_ms"] * 1e-3) / 1e12 / COPY_RATE_TBS, 3))
        st["export_variant"] = ctx.get_stat("export_variant")
        out["C_k_export_" + n] = st
    for n, d in pitched.items():
        ms = []
        for i in range(warmup + rounds):
            ctx.timing_reset()
            ctx.export([(n, d)])
            if i >= warmup:
                ms.append(ctx.timing_read()["k_export"][0])
        st, traffic = stats(ms), items[n][2]
        st.update(bytes_read_and_written=traffic, tb_per_s=round(traffic / (st["median_ms"] * 1e-3) / 1e12, 3),
                  share_of_copy_rate=round(traffic / (st["median_ms"] * 1e-3) / 1e12 / COPY_RATE_TBS, 3), export_variant=ctx.get_stat("export_variant"))
        out["C_k_export_%s_pitch%d" % (n, pitch)] = st
    ctx.timing_enable(0)
    # the exported buffers hold what the getters return
    idx, dist = ctx.get_topr()
    got = np.empty((Q, R), np.int64)
    producer.memcpy_dtoh(got, dst["idx"].ptr, got.nbytes)
    same = np.array_equal(got, idx.astype(np.int64))
    g8 = np.empty((Q, R), np.uint8)
    producer.memcpy_dtoh(g8, dst["dist"].ptr, g8.nbytes)
    same = same and np.array_equal(g8, dist)
    producer.memcpy_dtoh(g8, dst["match"].ptr, g8.nbytes)
    out["exports_equal_the_getters"] = bool(same and np.array_equal(g8, ctx.get_match()))
    print(json.dumps(out), flush=True)
    ctx.close()
    producer.close()
    if not out["exports_equal_the_getters"]:
        sys.exit(1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--shapes", default="c2,c3")
    p.add_argument("--limit", type=int, default=300, help="seconds a shape may take")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dev_output_timing.txt"))
    p.add_argument("--child", default=None)
    a = p.parse_args()
    if a.child:
        return child(a.child, a.rounds, a.warmup)
    lines = ["python tools/dev_output_timing.py --rounds %d --warmup %d --shapes %s" % (a.rounds, a.warmup, a.shapes), ""]
    recs = []
    for shape in a.shapes.split(","):
        env = dict(os.environ)
        env.pop("HG_LIBRARY", None)
        r = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--rounds", str(a.rounds),
                            "--warmup", str(a.warmup), "--child", shape], capture_output=True, text=True, env=env)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("shape %s ended with status %d: stopping" % (shape, r.returncode))
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        recs.append(rec)
        lines.append(json.dumps(rec))
    lines += ["", "%-5s %-34s %s" % ("shape", "leg", "median ms (min .. max of the rounds)")]
    for rec in recs:
        for leg in [k for k in rec if k[:2] in ("A_", "B_", "C_") and isinstance(rec[k], dict)]:
            v = rec[leg]
            extra = "   %.3f TB/s read + written, %.0f %% of the %.2f TB/s copy rate, %s path" % (
                v["tb_per_s"], 100 * v["share_of_copy_rate"], COPY_RATE_TBS, "16-byte" if v["export_variant"] == 1 else "element-wise") if "tb_per_s" in v else ""
            lines.append("%-5s %-34s %.4f (%.4f .. %.4f)%s" % (rec["shape"], leg, v["median_ms"], v["min_ms"], v["max_ms"], extra))
        lines.append("%-5s host route / export: %.1fx; exports equal the getters: %s" % (
            rec["shape"], rec["B_host_get_topr_get_match"]["median_ms"] / rec["A_export_idx64_dist_match"]["median_ms"], rec["exports_equal_the_getters"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
