"""Label-free relevance (hg_set_neighbours, hg_neighbours_from_lists, hg_match_neighbours, hg_nbr_hist) on resident tables at C2
(Q=10k, N=1M, b=64, R=5000) with G=1000 neighbours per query: the first G ranks of the Hamming ranking, columns shuffled.

  set_from_host   hg_set_neighbours (wall clock around the call: the Q x G x 4 byte upload, k_nbr_sort, the flag word back) and
                  k_nbr_sort's own HIP-event time
  from_lists      hg_neighbours_from_lists (wall clock; no upload) and k_nbr_sort's time on the strided slice of the lists
  match_ap_at     hg_match_neighbours + hg_ap_at at eight cut-offs (wall clock each), k_nbr_match's and k_ap_at's times, the getter
  nbr_hist        hg_nbr_hist (wall clock), k_nbr_hist's time, the getter
  host_route      what a caller did before: hg_get_topr (Q x R x 5 bytes over PCIe) + np.isin per query + the hit counts at the
                  cut-offs; compared with the device's

Every step is a process of its own under `timeout`, started one after the other; the first failure ends the run.  Medians of `--reps`
rounds after `--warmup` rounds; one JSON line per step (profiles/neighbour_timing.txt).

    python tools/neighbour_timing.py --out profiles/neighbour_timing.txt      # from the repository root, on an MI355X
"""
import argparse, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("set_from_host", "from_lists", "match_ap_at", "nbr_hist", "host_route")
KS = [1, 10, 50, 100, 500, 1000, 2500, 5000]
G = 1000


def med(x):
    return round(float(np.median(x)), 4) if len(x) else None


def kernel_ms(t, k):
    return t[k][0] / max(1, t[k][1])


def setup():
    from tests import cases
    from hashgan_amd import _native, metric
    spec = dict(cases.CASES["c2_q64"]); spec.pop("q_take", None)
    cases.CASES["_full"] = spec
    c = cases.build_case("_full")
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), c["b"], c["dblab"].shape[1])
    ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
    ctx.timing_enable(2)
    ctx.topr(c["R"])
    return ctx, c


def run_step(step, args):
    ctx, c = setup()
    Q, N, R = len(c["qbits"]), len(c["dbbits"]), c["R"]
    ks = np.array(KS, dtype=np.int64)
    rng = np.random.default_rng(1)
    s, extra = {}, {}

    def timed(name, fn, kernels=()):
        ctx.timing_reset()
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        t = ctx.timing_read() if kernels else {}
        if rep >= args.warmup:
            s.setdefault(name, []).append(dt)
            for k in kernels:
                s.setdefault(k, []).append(kernel_ms(t, k))
        return r

    if step in ("set_from_host", "host_route"):
        idx, _ = ctx.get_topr()
        gt = np.ascontiguousarray(idx[:, rng.permutation(G)])                # the first G ranks, in another order
    if step != "set_from_host":
        ctx.neighbours_from_lists(G)
    reps = args.warmup + (args.host_reps if step == "host_route" else args.reps)
    for rep in range(reps):
        if step == "set_from_host":
            timed("set_neighbours_wall", lambda: ctx.set_neighbours(gt), ("k_nbr_sort",))
        elif step == "from_lists":
            timed("neighbours_from_lists_wall", lambda: ctx.neighbours_from_lists(G), ("k_nbr_sort",))
        elif step == "match_ap_at":
            timed("match_neighbours_wall", ctx.match_neighbours, ("k_nbr_match",))
            timed("ap_at_wall", lambda: ctx.ap_at(ks), ("k_ap_at",))
            ap, hits = timed("get_ap_at_wall", ctx.get_ap_at)
            extra["hits_at_G_all_equal_G"] = bool((hits[:, KS.index(G)] == G).all())
        elif step == "nbr_hist":
            timed("nbr_hist_wall", ctx.nbr_hist, ("k_nbr_hist",))
            nbr, cnt = timed("get_nbr_hist_wall", ctx.get_nbr_hist)
            extra["columns_sum_to_G"] = bool((nbr.sum(0) == G).all() and (cnt == G).all())
        else:
            def host():
                idx, _ = ctx.get_topr()
                m = np.empty(idx.shape, dtype=bool)
                for q in range(Q):
                    m[q] = np.isin(idx[q], gt[q])
                return np.cumsum(m, axis=1)[:, ks - 1]
            hv = timed("host_wall", host)
            if rep == 0:
                ctx.match_neighbours()
                ctx.ap_at(ks)
                extra["hits_host_equal_device"] = bool(np.array_equal(hv, ctx.get_ap_at()[1]))
    from hashgan_amd import _native
    out = {"step": step, "case": "C2 (Q=10k, N=1M, b=64, R=5000), G=1000", "library": os.path.basename(_native.library_path()), "Q": Q, "N": N, "R": R,
           "G": G, "ks": KS, "ms_median": {k: med(v) for k, v in s.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in s.items()}}
    out.update(extra)
    if step == "set_from_host":
        out["set_bytes_over_pcie"] = Q * G * 4
    if step == "host_route":
        out["list_bytes_over_pcie"] = Q * R * 5
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--step", choices=STEPS, help="run one step in this process (the driver's children)")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds a step may take")
    ap.add_argument("--out", help="write the steps' JSON lines to this file")
    a = ap.parse_args()
    if a.step:
        run_step(a.step, a)
        sys.exit(0)
    lines = []
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--host-reps", str(a.host_reps)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            sys.exit("step %s ended with status %d: stopping" % (step, p.returncode))      # nothing more is started on the GPU
        lines.append(p.stdout)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(lines)
