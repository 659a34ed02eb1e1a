"""Class votes (hg_votes) on resident tables at C2 (Q=10k, N=1M, b=64, C=10 one-hot, R=5000), at the NUS-WIDE shape C3 (Q=2.1k, N=190k,
b=48, C=81 multi-hot, R=5000) and at the CIFAR evaluation (Q=1000, N=54k, b=32, C=10, R=N), eight cut-offs each, beside hg_graded at
the same cut-offs on the same lists in the same rounds -- the yardstick: it reads the same indices and gathers the same label words.
`--shapes ...,c2_one_class,cifar_one_class` adds the two shapes with every row in one class: every vote of a chunk goes to one counter.

  votes    hg_votes (wall clock around the call: the cut-offs' upload, k_votes, k_vote_confusion, one synchronisation), its two kernels'
           own HIP-event times, and the two small getters (pred / top and the confusion matrices)
  graded   hg_graded (wall clock) and k_graded's HIP-event time
  host     what a caller did before hg_votes: hg_get_topr (Q x R x 5 bytes over PCIe) + per query a NumPy gather of the label rows and
           their cumulative sums read at ks; compared with the device's votes
  ballot   only with the measurement build (HG_LIBRARY=.../libhashgan_amd_probe.so, python -m hashgan_amd.build --probes): k_votes
           counting by ballots instead of LDS adds (option "probe_votes" = 1; hg_votes.hpp) in the same rounds, its tables compared
           with the production form's

Medians of `--reps` rounds after `--warmup` rounds; one JSON line per shape (profiles/votes_timing.txt).

    python tools/votes_timing.py            # from the repository root, on an MI355X
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cases
from hashgan_amd import _native, metric
from hashgan_amd import extra_metrics as X

SHAPES = {"c2": ("c2_q64", "C2 (Q=10k, N=1M, b=64, C=10 one-hot, R=5000)", [1, 10, 50, 100, 500, 1000, 2500, 5000]),
          "nus": ("c3_nus_q64", "NUS-WIDE shape C3 (Q=2.1k, N=190k, b=48, C=81 multi-hot, R=5000)", [1, 10, 50, 100, 500, 1000, 2500, 5000]),
          "c2_one_class": ("c2_q64", "C2's codes, every row and query of class 0 (all the rows of a chunk vote for one counter)", [1, 10, 50, 100, 500, 1000, 2500, 5000]),
          "cifar_one_class": ("c1_cifar_full", "the CIFAR evaluation's codes, every row and query of class 0", [1, 10, 100, 1000, 5000, 10000, 25000, 54000]),
          "cifar": ("c1_cifar_full", "CIFAR evaluation (Q=1000, N=54k, b=32, C=10 one-hot, R=N)", [1, 10, 100, 1000, 5000, 10000, 25000, 54000])}


def full_case(name):
    spec = dict(cases.CASES[name]); spec.pop("q_take", None)
    cases.CASES["_full"] = spec
    return cases.build_case("_full")


def med(x):
    return round(float(np.median(x)), 4) if len(x) else None


def host_route(ctx, dl, ks):
    idx, _ = ctx.get_topr()
    out = np.empty((len(idx), len(ks), dl.shape[1]), dtype=np.uint32)
    for q in range(len(idx)):
        out[q] = np.cumsum(dl[idx[q]], axis=0, dtype=np.uint32)[ks - 1]
    return out


def run(key, args):
    name, label, ks = SHAPES[key]
    ks = np.array(ks, dtype=np.int64)
    c = full_case(name)
    qb, db, ql, dl = c["qbits"], c["dbbits"], c["qlab"], c["dblab"]
    if key.endswith("one_class"):
        ql, dl = np.zeros_like(ql), np.zeros_like(dl)
        ql[:, 0] = dl[:, 0] = 1
    Q, N, b, C = len(qb), len(db), c["b"], dl.shape[1]
    R = int(ks[-1])
    gain, disc = X.gain_table("linear", C), X.discount_table(R)
    ctx = _native.Context(0)
    ctx.set_database(metric.pack_codes(db), metric.pack_labels(dl), b, C)
    ctx.set_queries(metric.pack_codes(qb), metric.pack_labels(ql))
    try:
        ctx.set_option("probe_votes", 0)
        probes = True
    except _native.HashganNativeError:
        probes = False
    ctx.timing_enable(2)
    ctx.topr(R)                                                           # ranked once: both passes only read the lists
    names = ["votes_wall", "k_votes", "k_vote_confusion", "get_wall", "graded_wall", "k_graded", "host_wall"] + (["ballot_votes_wall", "k_votes_ballot"] if probes else [])
    s = {k: [] for k in names}
    same_host = same_ballot = None
    dl8 = np.ascontiguousarray(dl.astype(np.uint8))

    def kernel_ms(t, k):
        return t[k][0] / max(1, t[k][1])

    for rep in range(args.warmup + args.reps):
        timed = rep >= args.warmup
        for form in (("adds", "ballot") if probes else ("adds",)):      # alternating within the round
            if probes:
                ctx.set_option("probe_votes", int(form == "ballot"))
            ctx.timing_reset()
            t0 = time.perf_counter()
            ctx.votes(ks)
            t1 = time.perf_counter()
            t = ctx.timing_read()
            if form == "adds":
                pred, top = ctx.get_vote_pred()
                conf = ctx.get_vote_confusion()
                t2 = time.perf_counter()
                if timed:
                    s["votes_wall"].append((t1 - t0) * 1e3); s["get_wall"].append((t2 - t1) * 1e3)
                    s["k_votes"].append(kernel_ms(t, "k_votes")); s["k_vote_confusion"].append(kernel_ms(t, "k_vote_confusion"))
                if rep == 0:
                    votes = ctx.get_votes()
            else:
                if timed:
                    s["ballot_votes_wall"].append((t1 - t0) * 1e3); s["k_votes_ballot"].append(kernel_ms(t, "k_votes"))
                if rep == 0:
                    same_ballot = bool(np.array_equal(ctx.get_votes(), votes) and np.array_equal(ctx.get_vote_pred()[0], pred)
                                    and np.array_equal(ctx.get_vote_confusion(), conf))
        ctx.timing_reset()
        t0 = time.perf_counter()
        ctx.graded(ks, gain, disc)
        t1 = time.perf_counter()
        if timed:
            s["graded_wall"].append((t1 - t0) * 1e3); s["k_graded"].append(kernel_ms(ctx.timing_read(), "k_graded"))
        if rep >= args.warmup + args.reps - args.host_reps - 1 and args.host_reps:      # (one warm-up round of its own)
            t0 = time.perf_counter()
            hv = host_route(ctx, dl8, ks)
            t1 = time.perf_counter()
            same_host = bool(np.array_equal(hv, votes))
            if rep > args.warmup + args.reps - args.host_reps - 1:
                s["host_wall"].append((t1 - t0) * 1e3)
    m = {k: med(v) for k, v in s.items()}
    out = {"case": label, "library": os.path.basename(_native.library_path()), "Q": Q, "N": N, "b": b, "C": C, "R": R, "ks": ks.tolist(),
           "votes_host_equal_device": same_host, "ms_median": m, "ms_all": {k: [round(x, 4) for x in v] for k, v in s.items()},
           "list_bytes_over_pcie_host_route": Q * R * 5, "table_bytes_to_host_device_route": Q * len(ks) * 8 + len(ks) * C * C * 8,
           "accuracy_at_ks": [round(float(x), 4) for x in X.knn_from_tables(pred, conf, ql, ks)["accuracy"]],
           "ratio": {"k_votes / k_graded": round(m["k_votes"] / m["k_graded"], 3), "votes_wall / graded_wall": round(m["votes_wall"] / m["graded_wall"], 3)}}
    if m["host_wall"]:
        out["ratio"]["host_wall / (votes_wall + get_wall)"] = round(m["host_wall"] / (m["votes_wall"] + m["get_wall"]), 1)
    if probes:
        out["ballot_tables_equal_production"] = same_ballot
        out["ratio"]["k_votes_ballot / k_votes"] = round(m["k_votes_ballot"] / m["k_votes"], 3)
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--shapes", default="c2,nus,cifar")
    a = ap.parse_args()
    for key in a.shapes.split(","):
        run(key, a)
