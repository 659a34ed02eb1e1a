"""Kernel time of the relevant-row histogram (hg_rel_hist: k_hist_rel) against the plain full histogram pass on the same tables at C2 and
C3 -- k_hist through hg_hist, and k_hist_i8 through the one-shot exact sequence (optimistic = 0 with R x 8 <= N and N >= 65536 is
enqueue_exact_mx, whose do_hist(c, 1, true, true) launches k_hist_i8 under the timing name "k_hist"; the tool checks that exactly one
such launch was timed) -- the three alternating within one process: HIP events per kernel (timing level 2), medians of five rounds
after three warm-up rounds, one JSON line per shape.

    python tools/rel_hist_timing.py            # from the repository root, on an MI355X (profiles/rel_hist_timing.txt)

--joint: the distance-by-grade histogram instead (hg_joint_hist: k_label_max, k_hist_joint, k_hist_joint_reduce) against hg_rel_hist +
hg_grade_hist on the same resident tables -- together they read the same pairs and issue two LDS atomics per pair where the joint pass
issues one --, alternating within one process, the same medians; the joint table's two marginals are compared with the other two tables.

    python tools/rel_hist_timing.py --joint    # (profiles/joint_hist_timing.txt)
"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases
from hashgan_amd import _native, metric


def full_case(name):
    spec = dict(cases.CASES[name]); spec.pop("q_take", None)
    cases.CASES["_full"] = spec
    return cases.build_case("_full")


def med(x):
    return float(np.median(x))


def run(name, label):
    c = full_case(name)
    Q, N, b, C = c["qbits"].shape[0], c["dbbits"].shape[0], c["b"], c["dblab"].shape[1]
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), b, C)
    ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
    ctx.timing_enable(2)
    R = c["R"]
    series = {"rel_valu": [], "hist_valu": [], "hist_i8": [], "rel_valu_host": [], "rel_reduce_valu": [], "hist_reduce": []}
    variants = {}
    tables = {}
    for rep in range(8):                               # 3 warm-up rounds, 5 measured; the four versions alternate inside a round
        for key, hm in (("rel_valu", 0),):
            ctx.set_option("hist_mfma", hm)
            ctx.timing_reset()
            t0 = time.perf_counter()
            ctx.rel_hist()                             # (stage_sync = 1: returns after the stream has drained)
            t1 = time.perf_counter()
            t = ctx.timing_read()
            variants[key] = ctx.get_stat("rel_hist_variant")
            if rep >= 3:
                series[key].append(t["k_hist_rel"][0] / max(1, t["k_hist_rel"][1]))
                series["rel_reduce_" + key[4:]].append(t["k_hist_rel_reduce"][0] / max(1, t["k_hist_rel_reduce"][1]))
                series[key + "_host"].append((t1 - t0) * 1e3)
            if rep == 0:
                tables[key] = ctx.get_rel_hist()
        ctx.set_option("hist_mfma", 2)
        ctx.timing_reset()
        ctx.hist()                                     # the staged full pass: k_hist (vector ALU)
        t = ctx.timing_read()
        if rep >= 3:
            series["hist_valu"].append(t["k_hist"][0] / max(1, t["k_hist"][1]))
            series["hist_reduce"].append(t["k_hist_reduce"][0] / max(1, t["k_hist_reduce"][1]))
        if rep == 0:
            tables["hist"] = ctx.get_hist()
        ctx.set_option("optimistic", 0)                # the one-shot exact sequence: its full pass is k_hist_i8 per segment pair
        ctx.timing_reset()
        ctx.map(R)
        t = ctx.timing_read()
        ctx.set_option("optimistic", 1)
        assert t["k_hist"][1] == 1, t["k_hist"]         # (one full pass: the matrix-core exact sequence did not fall back)
        if rep >= 3:
            series["hist_i8"].append(t["k_hist"][0] / max(1, t["k_hist"][1]))
    same = bool(np.array_equal(tables["rel_valu"][0], tables["hist"]))
    out = {"case": label, "Q": Q, "N": N, "b": b, "C": C, "variants": variants, "all_equals_hg_hist": same,
           "ms_median": {k: round(med(v), 4) for k, v in series.items()}, "ms_all": {k: [round(x, 4) for x in v] for k, v in series.items()}}
    m = out["ms_median"]
    out["ratio"] = {"rel_valu / hist_valu": round(m["rel_valu"] / m["hist_valu"], 3), "rel_valu / hist_i8": round(m["rel_valu"] / m["hist_i8"], 3)}
    ctx.close()
    print(json.dumps(out), flush=True)


def run_joint(name, label):
    c = full_case(name)
    Q, N, b, C = c["qbits"].shape[0], c["dbbits"].shape[0], c["b"], c["dblab"].shape[1]
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(c["dbbits"]), metric.pack_labels(c["dblab"]), b, C)
    ctx.set_queries(metric.pack_codes(c["qbits"]), metric.pack_labels(c["qlab"]))
    ctx.timing_enable(2)
    kernels = ("k_label_max", "k_hist_joint", "k_hist_joint_reduce", "k_hist_rel", "k_hist_rel_reduce", "k_grade_hist", "k_grade_hist_reduce")
    series = {k: [] for k in kernels + ("joint_wall", "rel_wall", "grade_wall")}
    bytes0 = ctx.get_stat("device_bytes")
    for rep in range(8):                               # 3 warm-up rounds, 5 measured; the passes alternate inside a round
        ctx.timing_reset()
        t0 = time.perf_counter()
        ctx.joint_hist()                               # (stage_sync = 1: returns after the stream has drained)
        t1 = time.perf_counter()
        if rep == 0:
            joint_bytes = ctx.get_stat("device_bytes") - bytes0
        ctx.rel_hist()
        t2 = time.perf_counter()
        ctx.grade_hist()
        t3 = time.perf_counter()
        t = ctx.timing_read()
        assert all(t[k][1] == 1 for k in kernels), t
        if rep >= 3:
            for k in kernels:
                series[k].append(t[k][0])
            series["joint_wall"].append((t1 - t0) * 1e3); series["rel_wall"].append((t2 - t1) * 1e3); series["grade_wall"].append((t3 - t2) * 1e3)
    J = ctx.get_joint_hist()
    a, r = ctx.get_rel_hist()
    G = ctx.get_stat("joint_hist_grades")
    same = bool(np.array_equal(J.sum(1), a) and np.array_equal(J[:, 1:].sum(1), r) and np.array_equal(J.sum(0), ctx.get_grade_hist()[:G]))
    m = {k: round(med(v), 4) for k, v in series.items()}
    out = {"case": label, "Q": Q, "N": N, "b": b, "C": C, "grades": G, "bands": ctx.get_stat("joint_hist_bands"),
           "joint_buffers_MB": round(joint_bytes / 2 ** 20, 1), "marginals_equal_rel_hist_and_grade_hist": same, "ms_median": m,
           "ms_all": {k: [round(x, 4) for x in v] for k, v in series.items()}}
    out["kernels_ms"] = {"joint": round(m["k_label_max"] + m["k_hist_joint"] + m["k_hist_joint_reduce"], 4),
                         "rel + grade": round(m["k_hist_rel"] + m["k_hist_rel_reduce"] + m["k_grade_hist"] + m["k_grade_hist_reduce"], 4)}
    out["ratio"] = {"joint / (rel + grade), kernels": round(out["kernels_ms"]["joint"] / out["kernels_ms"]["rel + grade"], 3),
                    "joint / (rel + grade), wall": round(m["joint_wall"] / (m["rel_wall"] + m["grade_wall"]), 3)}
    ctx.close()
    print(json.dumps(out), flush=True)


for fn in ((run_joint,) if "--joint" in sys.argv[1:] else (run,)):
    fn("c2_q64", "C2 (Q=10k, N=1M, b=64, C=10 one-hot)")
    fn("c3_nus_q64", "C3 (Q=2.1k, N=190k, b=48, C=81 multi-hot)")
