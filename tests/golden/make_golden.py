#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the UNMODIFIED reference (run in the build
container only: it imports /root/reference/lib/metric.py, which never ships).

For every case in tests/cases.py the inputs are regenerated from the seed, the
+-1 features get one extra tie-breaking coordinate (oracle.tie_free_features,
SURVEY.md section 8c) so that the reference's np.argsort(-ips, 1) has no ties
to break, and `MAPs(R).get_maps_by_feature(database, query)` is called
  * once with all queries      -> `map`   (float64; nan if every query skipped)
  * once per single query row  -> `ap[i]` (np.mean of a 1-element list is the
    AP itself; nan marks a query the reference skips because rel == 0).
For the small cases the first R entries of np.argsort(-ips', 1) are stored too
(`idx`), pinning the canonical order itself.

Also extracts the CIFAR-10 class vectors from the reference's label lists
(data_list/cifar10/{database,test}.txt -- data files, stored as class indices), and records what
tests/test_oracle_vs_reference.py and tests/test_evalio.py compare with (reference_live.npz, reference_files.npz),
so that no test reads the reference itself.

Usage:  python tests/golden/make_golden.py [case ...]
"""
import os
import sys
import types
import warnings
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from lib.metric import MAPs            # the reference itself  (noqa: E402)
from oracle import hamming_map as O    # only tie_free_features is used here  (noqa: E402)


def cifar_labels():
    out = {}
    for split in ("database", "test"):
        rows = [l.split()[1:] for l in open(os.path.join(REF, "data_list/cifar10/%s.txt" % split))]
        lab = np.array(rows, dtype=np.int64)
        assert (lab.sum(1) == 1).all()
        out[split + "_cls"] = lab.argmax(1).astype(np.uint8)
    np.savez_compressed(os.path.join(HERE, "cifar10_labels.npz"), **out)


def run_case(name):
    from tests import cases
    c = cases.build_case(name)
    N, R = c["dbbits"].shape[0], c["R"]
    database = types.SimpleNamespace(output=O.tie_free_features(c["dbbits"], False, N),
                                     label=c["dblab"].astype(np.int64))
    qfeat = O.tie_free_features(c["qbits"], True, N)
    qlab = c["qlab"].astype(np.int64)
    Q = qfeat.shape[0]
    ap = np.empty(Q, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(Q):
            one = types.SimpleNamespace(output=qfeat[i:i + 1], label=qlab[i:i + 1])
            ap[i] = MAPs(R).get_maps_by_feature(database, one)
        if N * Q <= 60_000_000:
            allq = types.SimpleNamespace(output=qfeat, label=qlab)
            m = MAPs(R).get_maps_by_feature(database, allq)
        else:                                   # memory: same value by metric.py:24
            m = np.mean(np.array([a for a in ap if not np.isnan(a)]))
    out = dict(ap=ap, map=np.float64(m))
    if name in cases.SMALL:
        ips = np.dot(qfeat, database.output.T)
        out["idx"] = np.argsort(-ips, 1)[:, :R].astype(np.int64)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("%-16s Q=%-5d N=%-9d R=%-6d map=%.17g skipped=%d" % (name, Q, N, R, m, int(np.isnan(ap).sum())))


def run_real_case(name):
    """Real-valued features on the 1/64 grid (exact float arithmetic in any order): the unmodified
    reference on float64 copies + the tie-breaking coordinate (oracle.real_map.tie_free_real_features)."""
    from tests import cases
    from oracle import real_map as RM
    c = cases.build_real_case(name)
    N, R = c["dbf"].shape[0], c["R"]
    database = types.SimpleNamespace(output=RM.tie_free_real_features(c["dbf"], False, N), label=c["dblab"].astype(np.int64))
    qfeat = RM.tie_free_real_features(c["qf"], True, N)
    qlab = c["qlab"].astype(np.int64)
    Q = qfeat.shape[0]
    ap = np.empty(Q, dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(Q):
            one = types.SimpleNamespace(output=qfeat[i:i + 1], label=qlab[i:i + 1])
            ap[i] = MAPs(R).get_maps_by_feature(database, one)
        m = MAPs(R).get_maps_by_feature(database, types.SimpleNamespace(output=qfeat, label=qlab))
    out = dict(ap=ap, map=np.float64(m))
    if N * Q <= 2_000_000:
        out["idx"] = np.argsort(-np.dot(qfeat, database.output.T), 1)[:, :R].astype(np.int64)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("%-16s Q=%-5d N=%-9d R=%-6d map=%.17g skipped=%d" % (name, Q, N, R, m, int(np.isnan(ap).sum())))


def reference_live():
    """tests/test_oracle_vs_reference.py: the reference's mAP on that module's seeded cases (its LIVE_CASES), and the
    name of the exception it raises for R > N."""
    from tests import test_oracle_vs_reference as T
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for case in T.LIVE_CASES:
            *_, database, query = T.live_inputs(*case)
            out[T.live_key(*case)] = np.float64(MAPs(case[3]).get_maps_by_feature(database, query))
    d, q, R = T.r_gt_n_inputs()
    try:
        MAPs(R).get_maps_by_feature(d, q)
        out["r_gt_n_raises"] = np.array("")
    except Exception as e:      # noqa: BLE001 -- recorded, the test asserts which
        out["r_gt_n_raises"] = np.array(type(e).__name__)
    np.savez_compressed(os.path.join(HERE, "reference_live.npz"), **out)


def reference_files():
    """tests/test_evalio.py: data_list/cifar10/test.txt verbatim (a data file), and of two configuration files only the
    entries the evaluation reads (DATA.LABEL_DIM / DB_SIZE / TEST_SIZE / MAP_R, MODEL.HASH_DIM where set), re-emitted as YAML.
    Every file is stored as its bytes (uint8)."""
    import yaml
    out = {"cifar10_test.txt": open(os.path.join(REF, "data_list/cifar10/test.txt"), "rb").read()}
    for name in ("cifar_evaluation", "nuswide_step_1"):
        with open(os.path.join(REF, "config", name + ".yaml")) as f:
            y = yaml.safe_load(f)
        keep = {"DATA": {k: y["DATA"][k] for k in ("LABEL_DIM", "DB_SIZE", "TEST_SIZE", "MAP_R") if k in y["DATA"]}}
        if "HASH_DIM" in (y.get("MODEL") or {}):
            keep["MODEL"] = {"HASH_DIM": y["MODEL"]["HASH_DIM"]}
        out[name + ".yaml"] = yaml.safe_dump(keep).encode()
    np.savez_compressed(os.path.join(HERE, "reference_files.npz"), **{k: np.frombuffer(v, np.uint8) for k, v in out.items()})


if __name__ == "__main__":
    cifar_labels()
    reference_live()
    reference_files()
    from tests import cases
    names = sys.argv[1:] or (list(cases.CASES) + list(cases.REAL_CASES))
    for nm in names:
        (run_real_case if nm in cases.REAL_CASES else run_case)(nm)
