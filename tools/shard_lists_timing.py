"""Graded sums and class votes on a database split G ways, at C3 (Q=2100, N=190k, b=48, 81 multi-hot labels) and C2 (Q=10k, N=1M, b=64,
10 classes), R = 5000 and eight cut-offs, on ONE GPU: virtual shards (G threads, G contexts, sharded.LocalComm -- the gather is G
device-to-device copies, no wire: the exchange itself is NOT measured here), G = 1, 2, 4, 8.

Per G, after the exact staged ranking with lists (sharded.rank_lists_shard, timed as rank_wall):
  lists      rank 0's HIP-event times of the kernels of pack, merge and metric -- k_list_grades, k_list_merge_grades, k_graded (from the
             merged plane), k_votes (the owned-slots pack), k_list_merge_votes, k_vote_pick, k_vote_confusion -- and the slowest rank's
             wall clock of both pack + gather + merge + metric sequences together (lists_wall)
  host       what a caller has to do without them for the same numbers: evaluate_shard(..., gather_topr=True) -- every rank
             all-gathers Q x R x 5 bytes and downloads the merged lists (gather_topr_wall, slowest rank) -- and then the labels of the
             listed rows gathered with NumPy, grade sums and per-class counts at the cut-offs (host_labels_wall: one rank, one round, at the
             first G only -- the merged lists do not depend on G)

Medians of `--reps` rounds after `--warmup`; one JSON line per (case, G) (profiles/shard_lists_timing.txt).  The shards' tables are
compared with one context's in every round.

    python tools/shard_lists_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases
from hashgan_amd import _native, metric, sharded
from hashgan_amd import extra_metrics as X

KS = np.array([1, 10, 50, 100, 500, 1000, 2500, 5000], dtype=np.int64)
KERNELS = ("k_list_grades", "k_list_merge_grades", "k_graded", "k_votes", "k_list_merge_votes", "k_vote_pick", "k_vote_confusion")


def full_case(name):
    spec = dict(cases.CASES[name]); spec.pop("q_take", None)
    cases.CASES["_full"] = spec
    return cases.build_case("_full")


def med(x):
    return round(float(np.median(x)), 4)


def per_launch(t, k):
    return t[k][0] / max(1, t[k][1]) if k in t else 0.0


def host_tables(idx, ql, dl, ks):
    """Grade sums and per-class counts at the cut-offs from downloaded lists, NumPy only, 64 queries at a time: the label gather
    dl[idx], then sums over the ranks between two cut-offs."""
    votes = np.zeros((len(idx), len(ks), dl.shape[1]), dtype=np.int64)
    lo = np.concatenate([[0], ks[:-1]])
    for q0 in range(0, len(idx), 64):
        lab = dl[idx[q0:q0 + 64]]                                            # [q, R, C]
        for j in range(len(ks)):
            votes[q0:q0 + 64, j] = lab[:, lo[j]:ks[j]].sum(1, dtype=np.int64)
    votes = np.cumsum(votes, axis=1)
    return np.einsum("qjc,qc->qj", votes, ql.astype(np.int64)), votes


def run(label, c, G, args):
    qb, db, ql, dl = c["qbits"], c["dbbits"], c["qlab"], c["dblab"]
    Q, N, b, C, R = len(qb), len(db), c["b"], dl.shape[1], int(KS[-1])
    qc, qw = metric.pack_codes(qb), metric.pack_labels(ql)
    dc, dw = metric.pack_codes(db), metric.pack_labels(dl)
    gain, disc = X.gain_table("exp", C), X.discount_table(R)
    rounds = args.warmup + args.reps
    one = _native.Context(0)
    one.set_database(dc, dw, b, C)
    one.set_queries(qc, qw)
    one.topr(R)
    one.graded(KS, gain, disc)
    one.votes(KS)
    ref = (one.get_graded(), one.get_vote_pred(), one.get_vote_confusion())
    ref_gsum, ref_votes = ref[0][0], one.get_votes()
    one.close()

    bounds = sharded.shard_bounds(N, G)
    walls = np.zeros((rounds, G, 3))
    events, same, host_wall = [], [], []

    def work(r, comm):
        lo, n = bounds[r]
        ctx = _native.Context(0)
        ctx.set_database(dc[lo:lo + n], dw[lo:lo + n], b, C, idx_base=lo, n_total=N)
        ctx.set_queries(qc, qw)
        ctx.timing_enable(2)
        comm.ctx = ctx
        for rep in range(rounds):
            comm.barrier()
            t0 = time.perf_counter()
            sharded.rank_lists_shard(ctx, comm, R)
            ctx.synchronize()
            ctx.timing_reset()
            comm.barrier()
            t1 = time.perf_counter()
            sharded.merge_list_table(ctx, comm, "grades")
            ctx.graded(KS, gain, disc)
            sharded.merge_list_table(ctx, comm, "votes", KS)
            ctx.votes(KS)
            t2 = time.perf_counter()
            if r == 0:
                events.append(ctx.timing_read())
                got = (ctx.get_graded(), ctx.get_vote_pred(), ctx.get_vote_confusion())
                same.append(all(np.array_equal(a, b_, equal_nan=True) for x, y in zip(got, ref)
                                for a, b_ in (zip(x, y) if isinstance(x, tuple) else [(x, y)])))
            comm.barrier()
            t3 = time.perf_counter()
            engine = sharded.HipShardEngine(ctx, want_lists=True)
            idx = sharded.evaluate_shard(engine, comm, R, gather_topr=True, always_gather=True, bet=False)[2][0]
            t4 = time.perf_counter()
            walls[rep, r] = ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t4 - t3) * 1e3)
            if r == 0 and rep == rounds - 1 and G == args.shards[0]:       # (the lists, and so this figure, do not depend on G)
                t5 = time.perf_counter()
                gsum, votes = host_tables(idx, ql.astype(np.int8), dl.astype(np.int8), KS)
                host_wall.append((time.perf_counter() - t5) * 1e3)
                same.append(np.array_equal(gsum, ref_gsum) and np.array_equal(votes, ref_votes.astype(np.int64)))
            comm.barrier()
        ctx.close()

    sharded.LocalComm.run(G, work)
    keep = slice(args.warmup, rounds)
    Qpad, Rp, nk = (Q + 63) // 64 * 64, (R + 15) // 16 * 16, len(KS)
    out = {"case": label, "Q": Q, "N": N, "b": b, "C": C, "R": R, "cutoffs": nk, "shards": G,
           "grade_block_bytes": Q * Rp + 4 * Qpad, "vote_block_bytes": 4 * nk * (C + 1) * Qpad, "topr_bytes_per_rank": Q * R * 5,
           "kernels_ms_median": {k: med([per_launch(t, k) for t in events[keep]]) for k in KERNELS},
           "rank_wall_ms": med(walls[keep, :, 0].max(1)), "lists_wall_ms": med(walls[keep, :, 1].max(1)),
           "gather_topr_wall_ms": med(walls[keep, :, 2].max(1)), "host_labels_wall_ms": med(host_wall) if host_wall else None,
           "equals_one_context": bool(same) and all(same)}
    print(json.dumps(out), flush=True)


def main(args):
    for label, name in (("C3 (Q=2100, N=190k, b=48, 81 multi-hot labels)", "c3_nus_q64"), ("C2 (Q=10k, N=1M, b=64, 10 classes)", "c2_q64")):
        c = full_case(name)
        for G in args.shards:
            run(label, c, G, args)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--shards", type=int, nargs="+", default=[1, 2, 4, 8])
    main(p.parse_args())
