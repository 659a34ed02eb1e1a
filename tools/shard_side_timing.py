"""Tie-aware AP on a database split eight ways, next to the same call on one context, at C2 (Q=10k, N=1M, b=64, R=5000) on ONE GPU:
virtual shards (G threads, G contexts, sharded.LocalComm -- the gather is G device-to-device copies, no wire), alternating with the
one-context call within one process.

  one_context     hg_tie_ap on the whole database: tie_ap_cold_wall (the histogram pass k_hist_rel + k_hist_rel_reduce, then k_tie_ap),
                  tie_ap_warm_wall (k_tie_ap alone), and the kernels' own HIP-event times
  shards          per rank, the slowest rank's wall clock per round: shard_pass_wall (hg_rel_hist on N / G rows, the G ranks sharing the
                  GPU), merged_call_wall (hg_pack_side_table + comm.all_gather + hg_merge_side_table + hg_tie_ap, the pass's table being
                  there), and rank 0's HIP-event times of k_side_pack, k_side_merge, k_tie_ap

Medians of `--reps` rounds after `--warmup` rounds; one JSON line (profiles/shard_side_timing.txt).  The merged results are compared
with the one-context results bit for bit in every round.

    python tools/shard_side_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases
from hashgan_amd import _native, metric, sharded


def full_case(name):
    spec = dict(cases.CASES[name]); spec.pop("q_take", None)
    cases.CASES["_full"] = spec
    return cases.build_case("_full")


def med(x):
    return round(float(np.median(x)), 4)


def per_launch(t, k):
    return t[k][0] / max(1, t[k][1]) if k in t else 0.0


def main(args):
    c = full_case("c2_q64")
    qb, db, ql, dl = c["qbits"], c["dbbits"], c["qlab"], c["dblab"]
    Q, N, b, C, R, G = len(qb), len(db), c["b"], dl.shape[1], int(c["R"]), args.shards
    Rs = np.array([R], dtype=np.int64)
    qc, qw = metric.pack_codes(qb), metric.pack_labels(ql)
    dc, dw = metric.pack_codes(db), metric.pack_labels(dl)
    rounds = args.warmup + args.reps

    bounds = sharded.shard_bounds(N, G)
    walls = np.zeros((rounds, G, 2))
    events, same = [], []
    ref = {}
    s = {k: [] for k in ("tie_ap_cold_wall", "tie_ap_warm_wall", "k_hist_rel", "k_hist_rel_reduce", "k_tie_ap")}

    def one_context_round(one, rep):
        one.set_queries(qc, qw)
        one.synchronize()
        one.timing_reset()
        t0 = time.perf_counter()
        one.tie_ap(Rs)                                     # cold: no tables
        t1 = time.perf_counter()
        cold = one.timing_read()
        one.timing_reset()
        t2 = time.perf_counter()
        one.tie_ap(Rs)                                     # warm: the tables are there
        t3 = time.perf_counter()
        warm = one.timing_read()
        ref.update(one.get_tie_ap())
        if rep >= args.warmup:
            s["tie_ap_cold_wall"].append((t1 - t0) * 1e3); s["tie_ap_warm_wall"].append((t3 - t2) * 1e3)
            s["k_hist_rel"].append(per_launch(cold, "k_hist_rel")); s["k_hist_rel_reduce"].append(per_launch(cold, "k_hist_rel_reduce"))
            s["k_tie_ap"].append(per_launch(warm, "k_tie_ap"))

    def work(r, comm):
        lo, n = bounds[r]
        ctx = _native.Context(0)
        ctx.set_database(dc[lo:lo + n], dw[lo:lo + n], b, C, idx_base=lo, n_total=N)
        ctx.set_queries(qc, qw)
        ctx.timing_enable(2)
        comm.ctx = ctx
        if r == 0:                                         # rank 0 also makes the one-context call of every round, the others waiting
            one = _native.Context(0)
            one.set_database(dc, dw, b, C)
            one.set_queries(qc, qw)
            one.timing_enable(2)
        for rep in range(rounds):
            if r == 0:
                one_context_round(one, rep)
            comm.barrier()                                 # (the one-context call of this round is over)
            ctx.set_queries(qc, qw)                        # stale tables, like the one-context cold call
            ctx.synchronize()
            ctx.timing_reset()
            comm.barrier()
            t0 = time.perf_counter()
            ctx.rel_hist()
            t1 = time.perf_counter()
            comm.barrier()
            t2 = time.perf_counter()
            ptr, nbytes = ctx.pack_side_table("rel")
            gathered = comm.all_gather(sharded.DevBuf(ptr, nbytes))
            ctx.merge_side_table("rel", gathered.ptr, G)
            ctx.tie_ap(Rs)
            t3 = time.perf_counter()
            walls[rep, r] = ((t1 - t0) * 1e3, (t3 - t2) * 1e3)
            if r == 0:
                events.append(ctx.timing_read())
                got = ctx.get_tie_ap()
                same.append(all(np.array_equal(got[k], ref[k], equal_nan=True) for k in ref))
            comm.barrier()                                 # (the shards' round is over)
        ctx.close()
        if r == 0:
            one.close()

    sharded.LocalComm.run(G, work)
    keep = slice(args.warmup, rounds)
    sh = {"shard_pass_wall": list(walls[keep, :, 0].max(1)), "merged_call_wall": list(walls[keep, :, 1].max(1))}
    for k in ("k_hist_rel", "k_side_pack", "k_side_merge", "k_tie_ap"):
        sh[k] = [per_launch(t, k) for t in events[keep]]
    out = {"case": "C2 (Q=10k, N=1M, b=64, C=10 one-hot, R=5000)", "Q": Q, "N": N, "b": b, "R": R, "shards": G,
           "gathered_bytes": G * 2 * (b + 1) * ((Q + 63) // 64 * 64) * 4,
           "one_context_ms_median": {k: med(v) for k, v in s.items()}, "shards_ms_median": {k: med(v) for k, v in sh.items()},
           "one_context_ms_all": {k: [round(x, 3) for x in v] for k, v in s.items()},
           "shards_ms_all": {k: [round(float(x), 3) for x in v] for k, v in sh.items()},
           "merged_equals_one_context": bool(same) and all(same)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--shards", type=int, default=8)
    main(p.parse_args())
