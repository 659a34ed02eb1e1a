"""AP, precision and recall at many cut-offs from one ranking (hg_ap_at) at C2 (Q=10k, N=1M, b=64), ks = 100 .. 5000 step 100,
against the two ways a caller had before, alternating within one process, medians of `--reps` rounds after `--warmup` rounds:

  one_pass       topr(max(ks)) + ap_at(ks) + get_ap_at() on resident tables: wall clock, with topr's and k_ap_at's own shares
                 (k_ap_at: HIP-event time from the timing table)
  parent_hits    what precision_recall_at_k did before this pass existed, on the same resident tables: topr(max(ks)) + get_match()
                 (Q x kmax bytes expanded on the host) + NumPy cumsum + pick -- hits only, no AP
  map_x50        one hg_map per cut-off: 50 calls, every one a pass over the Q x N pairs
  prk_now / prk_parent    extra_metrics.precision_recall_at_k end to end (loads included) as it is now and with the parent's body

Checked while timing: the hits of all three agree, and ap_at's column j has the bits of hg_map at ks[j].  One JSON line
(profiles/ap_at_timing.txt).

    python tools/ap_at_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases
from hashgan_amd import _native, metric
from hashgan_amd import extra_metrics as X


def full_case(name):
    spec = dict(cases.CASES[name]); spec.pop("q_take", None)
    cases.CASES["_full"] = spec
    return cases.build_case("_full")


def med(x):
    return round(float(np.median(x)), 4)


def parent_precision_recall_at_k(q_codes, db_codes, q_labels, db_labels, ks, device=0):
    """precision_recall_at_k as it was before hg_ap_at: the match bytes come to the host and are summed there."""
    ks = np.asarray(sorted(int(k) for k in ks), dtype=np.int64)
    eng = metric._Shared.get(device)
    with eng.lock:
        ctx = X._load(eng, q_codes, db_codes, q_labels, db_labels)
        ctx.topr(int(ks[-1]))
        match = ctx.get_match()
        total_rel = X._tables(ctx)[1].sum(1)
    cum = np.cumsum(match.astype(np.int64), axis=1)
    hits = cum[:, ks - 1]
    precision = (hits / ks[None, :]).mean(0)
    ok = total_rel > 0
    recall = (hits[ok] / total_rel[ok, None]).mean(0) if ok.any() else np.full(len(ks), np.nan)
    return precision, recall


def run(args):
    c = full_case("c2_q64")
    qb, db, ql, dl = c["qbits"], c["dbbits"], c["qlab"], c["dblab"]
    Q, N, b, C = len(qb), len(db), c["b"], dl.shape[1]
    ks = np.arange(100, 5001, 100, dtype=np.int64)
    kmax = int(ks[-1])
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), b, C)
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
    keys = ("one_pass_wall", "topr_wall", "ap_at_wall", "get_ap_at_wall", "k_ap_at", "parent_hits_wall", "get_match_wall", "map_x50_wall")
    s = {k: [] for k in keys}
    ap = hits = hits_parent = None
    for rep in range(args.warmup + args.reps):
        ctx.timing_enable(0)
        t0 = time.perf_counter()
        ctx.topr(kmax)
        t1 = time.perf_counter()
        ctx.ap_at(ks)
        t2 = time.perf_counter()
        ap, hits = ctx.get_ap_at()
        t3 = time.perf_counter()
        ctx.timing_enable(2)                             # the kernel's own time, in a pass of its own
        ctx.timing_reset()
        ctx.ap_at(ks)
        ctx.synchronize()
        tk = ctx.timing_read()
        assert tk["k_ap_at"][1] == 1 and "k_ap" not in {k for k, (ms, n) in tk.items() if n}
        ctx.timing_enable(0)
        t4 = time.perf_counter()
        ctx.topr(kmax)
        t5 = time.perf_counter()
        match = ctx.get_match()
        t6 = time.perf_counter()
        hits_parent = np.cumsum(match.astype(np.int64), axis=1)[:, ks - 1]
        t7 = time.perf_counter()
        del match
        t8 = time.perf_counter()
        maps = [ctx.map(int(k)) for k in ks]
        t9 = time.perf_counter()
        if rep >= args.warmup:
            s["one_pass_wall"].append((t3 - t0) * 1e3); s["topr_wall"].append((t1 - t0) * 1e3)
            s["ap_at_wall"].append((t2 - t1) * 1e3); s["get_ap_at_wall"].append((t3 - t2) * 1e3)
            s["k_ap_at"].append(tk["k_ap_at"][0])
            s["parent_hits_wall"].append((t7 - t4) * 1e3); s["get_match_wall"].append((t6 - t5) * 1e3)
            s["map_x50_wall"].append((t9 - t8) * 1e3)
    same_hits = bool(np.array_equal(hits, hits_parent) and all(np.array_equal(hits[:, j], maps[j][1]) for j in range(len(ks))))
    same_ap = bool(all(np.array_equal(ap[:, j], maps[j][0], equal_nan=True) for j in range(len(ks))))
    ctx.close()
    e = {"prk_now_wall": [], "prk_parent_wall": []}
    p_now = p_par = None
    for rep in range(args.e2e_warmup + args.e2e_reps):
        t0 = time.perf_counter()
        p_now = X.precision_recall_at_k(qb, db, ql, dl, ks)
        t1 = time.perf_counter()
        p_par = parent_precision_recall_at_k(qb, db, ql, dl, ks)
        t2 = time.perf_counter()
        if rep >= args.e2e_warmup:
            e["prk_now_wall"].append((t1 - t0) * 1e3); e["prk_parent_wall"].append((t2 - t1) * 1e3)
    s.update(e)
    m = {k: med(v) for k, v in s.items()}
    out = {"case": "C2 (Q=10k, N=1M, b=64, C=10 one-hot), ks = 100 .. 5000 step 100 (50 cut-offs)", "Q": Q, "N": N, "b": b, "C": C,
           "reps": args.reps, "e2e_reps": args.e2e_reps, "ms_median": m, "ms_all": {k: [round(x, 3) for x in v] for k, v in s.items()},
           "hits_agree": same_hits, "ap_bits_equal_hg_map": same_ap,
           "prk_bits_equal_parent": bool(np.array_equal(p_now[0], p_par[0]) and np.array_equal(p_now[1], p_par[1], equal_nan=True)),
           "sum_last_chunk_over_Rmax": round(float((ks % 8192).sum()) / kmax, 3),
           "ratio": {"parent_hits_wall / one_pass_wall": round(m["parent_hits_wall"] / m["one_pass_wall"], 2),
                     "map_x50_wall / one_pass_wall": round(m["map_x50_wall"] / m["one_pass_wall"], 2),
                     "prk_parent_wall / prk_now_wall": round(m["prk_parent_wall"] / m["prk_now_wall"], 2)}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--e2e-reps", type=int, default=20)
    p.add_argument("--e2e-warmup", type=int, default=1)
    run(p.parse_args())
