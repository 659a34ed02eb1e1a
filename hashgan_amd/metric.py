"""Drop-in for HashGAN's retrieval metric on MI355X.

Mirrors /root/reference/lib/metric.py:4-24

    MAPs(R).get_maps_by_feature(database, query)        # main.py:26,164 -- database first

plus the spellings BASELINE.json's north star names (query first):

    MAP(query_codes, db_codes, query_labels, db_labels, R)
    calc_map(query_codes, db_codes, query_labels, db_labels, R)

MAPs ranks what the reference ranks: np.argsort(-np.dot(q, db.T)) (metric.py:13-14), ties broken
by ascending database index.  For +-1 codes that is ascending Hamming distance and runs on the
Hamming kernels; anything else -- HashGAN's real-valued tanh outputs, {0,1} bits (whose np.dot
counts common ones: NOT a Hamming ranking), codes containing zeros -- is ranked by float32 inner
product (`binarize=True` applies sign() first instead).  MAP / calc_map take binary codes only,
{0,1} bits or +-1, and rank by Hamming distance.  Labels are {0,1} matrices.  All ranking work
runs in the HIP kernels behind hashgan_amd._native; the host only checks arguments and takes the
final mean (metric.py:24).

Every array argument may also lie in GPU memory -- a torch tensor on the device, anything with
__cuda_array_interface__, a devarray.DeviceArray: it is then packed on the GPU straight out of the
caller's memory (devarray.as_device_array decides; INTEGRATION.md has the stream rule).  Database and
queries may be on different sides; the features and labels of one table must be on the same side.
"""
import threading

import numpy as np

from . import _native
from .devarray import DeviceArray, as_device_array, as_device_output


# ------------------------------------------------------------------ packing
def pack_codes(x):
    """[n, b] array -> uint64 [n, ceil(b/64)]; bit j = (x[:, j] > 0), little endian."""
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("codes must be a 2-D [n, b] array")
    n, b = x.shape
    W = (b + 63) // 64
    bits = np.zeros((n, W * 64), dtype=np.uint8)
    bits[:, :b] = x > 0
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n, W)


def pack_labels(lab):
    """{0,1} label matrix [n, C] -> uint64 [n, ceil(C/64)]."""
    lab = np.asarray(lab)
    if lab.ndim != 2 or lab.shape[1] < 1:
        raise ValueError("labels must be a 2-D [n, C] array")
    if not np.isin(lab, (0, 1)).all():
        raise ValueError("labels must be {0,1} indicator matrices")
    n, C_ = lab.shape
    LW = (C_ + 63) // 64
    bits = np.zeros((n, LW * 64), dtype=np.uint8)
    bits[:, :C_] = lab != 0
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(n, LW)


# ------------------------------------------------------------------ engine
class RetrievalEngine:
    """A database shard resident on one GPU, evaluated against query batches."""

    def __init__(self, device=0):
        self.ctx = _native.Context(device)
        self.b = self.C = self.N = self.db_kind = self.db_src = None
        self.resident = None           # _evaluate's shortcut: (codes, labels, mode) of the arrays whose packed copy is on the GPU

    def close(self):
        self.ctx.close()

    def forget(self):
        """Before the engine goes back to the pool: nothing of the last owner's tables may be taken for resident."""
        self.b = self.C = self.N = self.db_kind = self.db_src = None
        self.resident = None

    def set_database(self, codes, labels, idx_base=0, n_total=None, packed=False):
        if packed:
            cw, lw, b, C_ = codes
            lab = labels
        else:
            codes = np.asarray(codes)
            b = codes.shape[1]
            C_ = np.asarray(labels).shape[1]
            cw, lab = pack_codes(codes), pack_labels(labels)
        self.ctx.set_database(cw, lab, b, C_, idx_base, n_total)
        self.b, self.C = b, C_

    def set_database_packed(self, code_words, label_words, b, C_, idx_base=0, n_total=None):
        self.ctx.set_database(code_words, label_words, b, C_, idx_base, n_total)
        self.b, self.C = b, C_

    def set_queries(self, codes, labels):
        codes = np.asarray(codes)
        labels = np.asarray(labels)
        if codes.shape[1] != self.b or labels.shape[1] != self.C:
            raise ValueError("query codes/labels do not match the database (b=%s, C=%s)" % (self.b, self.C))
        self.ctx.set_queries(pack_codes(codes), pack_labels(labels))

    def set_queries_packed(self, code_words, label_words):
        self.ctx.set_queries(code_words, label_words)

    def average_precisions(self, R):
        """-> (ap float64 [Q] with nan where the query has no hit in its top R, rel int64 [Q])."""
        return self.ctx.map(R)

    def topr(self, R):
        self.ctx.topr(R)
        return self.ctx.get_topr()


def mean_over_hits(ap, rel):
    """metric.py:22-24: queries without a hit are skipped; mean of the rest
    (nan + RuntimeWarning if none is left, like np.mean of an empty array)."""
    if rel.size and rel.min() > 0:         # every query has a hit: the selection would be a copy of ap in the same order
        return np.mean(ap)
    return np.mean(np.array(ap[rel != 0]))


# ------------------------------------------------------------------ engines
class _Pool:
    """Process-wide pool of GPU contexts for MAPs objects.  main.py:164 writes `MAPs(cfg.DATA.MAP_R).get_maps_by_feature(...)`:
    a NEW object per evaluation, never closed.  A context of its own per object would mean a stream, ~0.3 GB of device buffers
    and the pinned staging blocks created and torn down around every call (hipMalloc / hipHostMalloc / hipFree: tens of
    milliseconds, and now and then a stall of a second -- bench.py's `drop_in_literal` leg).  So an object BORROWS a context on
    first use and hands it back when it is closed or collected; the context keeps its buffers (they only grow), the next
    object's tables are loaded into them.  An object that is alive keeps its context to itself (no two objects ever share
    device state at the same time); a context whose engine options were changed by its borrower is destroyed instead of
    recycled; at most `max_idle` contexts per device wait in the pool."""
    lock = threading.Lock()
    idle = {}
    max_idle = 2
    created = 0
    recycled = 0
    closed = 0

    @classmethod
    def acquire(cls, device):
        with cls.lock:
            lst = cls.idle.get(device)
            if lst:
                cls.recycled += 1
                return lst.pop()
            cls.created += 1
        eng = RetrievalEngine(device)
        eng.ctx.preload()          # (the process's first evaluation pays for every path's first use: no later one does)
        return eng

    @classmethod
    def release(cls, eng):
        keep = False
        try:
            touched = eng.ctx.options_touched - {"keep_floats", "keep_query_floats"}         # (set by every load / by _rank to what its mode needs)
            pending = getattr(eng.ctx, "_in_flight", None)
            if not touched and not pending and eng.ctx._h and not getattr(eng, "poisoned", False):
                eng.forget()
                with cls.lock:
                    lst = cls.idle.setdefault(eng.ctx.device, [])
                    if len(lst) < cls.max_idle:
                        lst.append(eng)
                        keep = True
        finally:
            if not keep:
                with cls.lock:
                    cls.closed += 1
                eng.close()

    @classmethod
    def close_all(cls):
        with cls.lock:
            engines = [e for lst in cls.idle.values() for e in lst]
            cls.idle.clear()
            cls.closed += len(engines)
        for e in engines:
            e.close()

    @classmethod
    def stats(cls):
        with cls.lock:
            idle = [e for lst in cls.idle.values() for e in lst]
            return {"contexts_created": cls.created, "contexts_recycled": cls.recycled, "contexts_closed": cls.closed,
                    "contexts_idle": len(idle), "idle_device_bytes": sum(e.ctx.get_stat("device_bytes") for e in idle)}


def pool_stats():
    """Counters of the MAPs context pool: contexts created / recycled / closed / idle, device bytes the idle ones hold."""
    return _Pool.stats()


class _Shared:
    """One lazily created engine per device for the function spellings (MAP, calc_map, extra_metrics): a context
    is not thread safe, so every use holds its lock.  MAPs objects borrow theirs from _Pool instead."""
    lock = threading.Lock()
    engines = {}

    @classmethod
    def get(cls, device):
        with cls.lock:
            if device not in cls.engines:
                e = RetrievalEngine(device)
                e.lock = threading.RLock()
                cls.engines[device] = e
            return cls.engines[device]

    @classmethod
    def close_all(cls):
        with cls.lock:
            for e in cls.engines.values():
                e.close()
            cls.engines.clear()


def release_engines():
    """Free the GPU contexts (and their device memory) behind MAP / calc_map / extra_metrics and the idle ones of MAPs' pool,
    and hand the library's cache of device and pinned blocks back to the HIP runtime."""
    _Shared.close_all()
    _Pool.close_all()
    _native.release_cache()


def _sides(codes, labels, what):
    """One table's (features, labels) as the loaders take them: two DeviceArray descriptors (device memory: never handed to
    np.asarray) or two ndarrays."""
    dc, dl = as_device_array(codes), as_device_array(labels)
    if (dc is None) != (dl is None):
        raise ValueError("%s features and labels must be on the same side: both in device memory or both on the host "
                         "(features on the %s, labels on the %s)" % (what, "device" if dc is not None else "host",
                                                                     "device" if dl is not None else "host"))
    if dc is not None:
        return dc, dl
    return np.asarray(codes), np.asarray(labels)


class PQTable:
    """A product-quantised database as the loaders see it: the stand-in for database.output in 'quantised' mode.  It has the decoded
    table's shape and nothing of its contents (codes uint8 [N, M], codebooks float32 [M, K, dsub]: hashgan_amd/pq.py)."""

    def __init__(self, codes, codebooks):
        from . import pq
        if as_device_array(codes) is not None or as_device_array(codebooks) is not None:
            raise ValueError("quantised=True takes codes and codebooks as host arrays")
        self.codes, self.codebooks = pq.check_tables(codes, codebooks, values=False)
        self.kept = (codes, codebooks)                 # the caller's own objects: what "the same arrays as last time" compares
        self.ndim = 2
        self.shape = (self.codes.shape[0], self.codebooks.shape[0] * self.codebooks.shape[2])

    def same_readonly(self, other):
        return (isinstance(other, PQTable) and self.kept[0] is other.kept[0] and self.kept[1] is other.kept[1]
                and not any(getattr(getattr(a, "flags", None), "writeable", True) for a in self.kept))


class PQFeatures:
    """A database to be product-quantised on the way in: float features [N, M * dsub] -- a host array, or a DeviceArray -- and the
    codebooks float32 [M, K, dsub] that the GPU assigns every row to (hg_set_database_pq_f32; device features: hg_pq_encode_dev, then
    hg_set_database_pq).  The loaders' other stand-in for database.output in 'quantised' mode, next to PQTable."""

    def __init__(self, features, codebooks):
        from . import pq
        if as_device_array(codebooks) is not None:
            raise ValueError("quantised=True takes the codebooks as a host array")
        self.codebooks = pq.check_codebooks(codebooks)
        dev = as_device_array(features)
        self.features = dev if dev is not None else np.asarray(features)
        if dev is None and self.features.dtype.kind != "f":
            raise ValueError("features must be floating point (have %s)" % self.features.dtype)
        self.kept = (features, codebooks)              # the caller's own objects: what "the same arrays as last time" compares
        self.ndim = self.features.ndim
        b = self.codebooks.shape[0] * self.codebooks.shape[2]
        if self.ndim != 2 or self.features.shape[1] != b:
            raise ValueError("features must be [N, M * dsub] = [N, %d] (have shape %r)" % (b, tuple(self.features.shape)))
        self.shape = (self.features.shape[0], b)

    def same_readonly(self, other):
        return (isinstance(other, PQFeatures) and self.kept[0] is other.kept[0] and self.kept[1] is other.kept[1]
                and not isinstance(self.features, DeviceArray)           # (nothing says device memory is unchanged)
                and not any(getattr(getattr(a, "flags", None), "writeable", True) for a in self.kept))


def _check_shapes(q_codes, db_codes, q_labels, db_labels, R):
    if db_codes.ndim != 2 or q_codes.ndim != 2 or db_codes.shape[1] != q_codes.shape[1]:
        raise ValueError("query and database codes must be [n, b] with the same b")
    if db_labels.ndim != 2 or q_labels.ndim != 2 or db_labels.shape[1] != q_labels.shape[1]:
        raise ValueError("query and database labels must be [n, C] with the same C")
    if db_labels.shape[0] != db_codes.shape[0] or q_labels.shape[0] != q_codes.shape[0]:
        raise ValueError("codes and labels must have the same number of rows")
    N = db_codes.shape[0]
    if not 1 <= R <= N:
        # metric.py:21 fails the same way: a length-N px cannot be divided by arange(1, R+1)
        raise ValueError("R=%d must be in 1..N (N=%d database rows)" % (R, N))


MAX_CUTOFFS = 64       # cut-offs one hg_ap_at pass takes


def _check_cutoffs(Rs, N, what="Rs"):
    """-> int64 array: 1..MAX_CUTOFFS strictly ascending integer cut-offs, each in 1..N (N None: no upper bound yet)."""
    Rs = np.asarray(Rs)
    if Rs.ndim != 1 or Rs.size == 0:
        raise ValueError("%s must be a non-empty list of cut-offs" % what)
    if Rs.dtype.kind not in "iu":
        raise ValueError("%s must be integers" % what)
    Rs = Rs.astype(np.int64)
    if Rs.size > MAX_CUTOFFS:
        raise ValueError("at most %d cut-offs per call (have %d)" % (MAX_CUTOFFS, Rs.size))
    if (np.diff(Rs) <= 0).any():
        raise ValueError("%s must be strictly ascending" % what)
    if Rs[0] < 1 or (N is not None and Rs[-1] > N):
        raise ValueError("every cut-off must be in 1..N")
    return Rs


def _ap_at(ctx, Rs, real, rerank=False, asym=False, quantised=False):
    """One ranking at the largest cut-off, then every cut-off from its match bitmap (hg_ap_at) -> (ap [Q, nR], rel [Q, nR])."""
    if rerank:
        ctx.topr_rerank(int(Rs[-1]), download=False)
    elif quantised:
        ctx.topr_pq(int(Rs[-1]), download=False)
    elif asym:
        ctx.topr_asym(int(Rs[-1]), download=False)
    elif real:
        ctx.topr_real(int(Rs[-1]), download=False)
    else:
        ctx.topr(int(Rs[-1]))
    ctx.ap_at(Rs)
    return ctx.get_ap_at()


def _kind(ctx, which):
    """What hg_set_*_f32 found in a float table: 'ones' (every entry +1: reads as either spelling), 'pm1' (every
    entry +-1), 'bits' (every entry 0/1), 'ternary' (-1/0/+1 mixed) or 'real'."""
    other, zeros, neg, _ = ctx.census(which)
    if other:
        return "real"
    if not zeros:
        return "pm1" if neg else "ones"
    return "bits" if not neg else "ternary"


def _load_database(eng, db_codes, db_labels, mode="reference", floats=None):
    """Host arrays: pack on the host, upload (hg_set_database_f32); DeviceArray descriptors: packed on the GPU out of the caller's
    memory (hg_set_database_dev; 'reference' mode keeps the floats at once).  The float table itself goes to the GPU only when it may be ranked
    by inner product: never for the spellings that binarise or insist on binary codes, and in 'reference' mode only if
    the database is not a +-1 code (a +-1 database meeting real-valued queries is uploaded again with it, below); 'rerank' mode always
    keeps it (keep_floats = 1): the floats order the rows inside equal Hamming distances; 'asymmetric' mode never does (keep_floats = 0:
    the loader signs the database, its floats never go to the GPU -- or, for device arrays, are never copied); 'quantised' mode hands a
    PQTable's codes and codebooks to hg_set_database_pq: no float table exists, on either side of PCIe."""
    eng.b = eng.C = eng.N = eng.db_kind = eng.db_src = None      # nothing is resident until this load has succeeded
    eng.resident = None                               # whoever loads another database (extra_metrics, MAPs) ends _evaluate's shortcut
    on_device = isinstance(db_codes, DeviceArray)
    if isinstance(db_codes, (PQTable, PQFeatures)) != (mode == "quantised"):
        raise ValueError("quantised=True ranks a database given as .codes / .codebooks, and only such a one")
    if mode == "quantised" and isinstance(db_codes, PQFeatures):
        # features to be encoded on the GPU: host arrays in one call; device arrays are encoded where they lie and the codes loaded
        if isinstance(db_codes.features, DeviceArray):
            codes, _, bad_rows = eng.ctx.pq_encode(db_codes.features, db_codes.codebooks)
            if bad_rows:
                raise ValueError("%d feature rows are not finite" % bad_rows)
            bad_c, bad_l = eng.ctx.set_database_pq(codes, db_codes.codebooks, db_labels)
        else:
            bad_c, bad_l = eng.ctx.set_database_pq_f32(db_codes.features, db_codes.codebooks, db_labels)
    elif mode == "quantised":
        bad_c, bad_l = eng.ctx.set_database_pq(db_codes.codes, db_codes.codebooks, db_labels)
    elif on_device:
        # device arrays: in 'reference' mode the floats are kept at once (a copy inside the GPU's memory, no PCIe) -- the caller's
        # memory may have changed by the time real-valued queries would ask for a second load, so there is none
        eng.ctx.set_option("keep_floats", floats if floats is not None else (1 if mode in ("reference", "rerank") else 0))
        bad_c, bad_l = eng.ctx.set_database_dev(db_codes, db_labels)
    else:
        eng.ctx.set_option("keep_floats", floats if floats is not None else (1 if mode == "rerank" else 2 if mode == "reference" else 0))
        bad_c, bad_l = eng.ctx.set_database_f32(db_codes, db_labels)
    if bad_l:
        raise ValueError("labels must be {0,1} indicator matrices")
    eng.b, eng.C = db_codes.shape[1], db_labels.shape[1]
    eng.db_kind = _kind(eng.ctx, 0)
    eng.N = db_codes.shape[0]
    eng.db_src = None if on_device else (db_codes, db_labels)     # for that second upload (host arrays only)


def _set_queries(eng, q_codes, q_labels):
    if isinstance(q_codes, DeviceArray):
        return eng.ctx.set_queries_dev(q_codes, q_labels)
    return eng.ctx.set_queries_f32(q_codes, q_labels)


def _rank(eng, q_codes, q_labels, R, mode, Rs=None, lists=False):
    """Queries against the engine's resident database -> (ap [Q], rel [Q]) at R, or with Rs (ascending cut-offs, R ignored)
    (ap [Q, nR], rel [Q, nR]) from one ranking at Rs[-1] (_ap_at); lists=True: the ranking at R with its lists left on the device
    (topr, topr_real or topr_rerank: what rank_into exports) -> "hamming" | "inner_product" | "rerank".  mode:
       'reference'  MAPs: what np.dot ranks (metric.py:13-14).  +-1 codes on both sides -> Hamming kernels (the same
                    order, ties by index); anything else -- real-valued tanh outputs, {0,1} bits (np.dot counts common
                    ones, not a Hamming distance), codes with zeros -- goes through the float32 inner-product ranking;
       'sign'       MAPs(binarize=True): sign() first, then Hamming;
       'codes'      MAP / calc_map (north-star spelling): binary codes only, {0,1} bits or +-1, ranked by Hamming
                    distance; anything else is an error;
       'rerank'     MAPs(rerank=True): sign() first, Hamming distance, then the float32 inner product of the features inside
                    equal distances, then the index (hg_topr_rerank): both float tables are on the GPU (_load_database);
       'asymmetric' MAPs(asymmetric=True): the queries' float32 features against the database's sign() codes read as +-1
                    (hg_topr_asym / hg_map_asym): the queries keep their floats on the GPU (keep_query_floats = 1), the database none;
       'quantised'  MAPs(quantised=True): the queries' float32 features against the database's product-quantisation codes
                    (hg_topr_pq / hg_map_pq), the queries' floats kept like the asymmetric mode's."""
    want_qf = 1 if mode in ("asymmetric", "quantised") else 0         # (set only when it changes: every hg_set_option ends hg_map_begin's licence to enqueue blind)
    if eng.ctx.option_values.get("keep_query_floats", 0) != want_qf:
        eng.ctx.set_option("keep_query_floats", want_qf)
    qbad_c, qbad_l = _set_queries(eng, q_codes, q_labels)
    if qbad_l:
        raise ValueError("labels must be {0,1} indicator matrices")
    if mode == "quantised":
        if lists:
            eng.ctx.topr_pq(R, download=False)
            return "inner_product"
        return eng.ctx.map_pq(R) if Rs is None else _ap_at(eng.ctx, Rs, True, quantised=True)
    if mode == "asymmetric":
        if q_codes.shape[1] > 255:
            raise ValueError("inner-product ranking supports up to 255 features (have %d)" % q_codes.shape[1])
        if lists:
            eng.ctx.topr_asym(R, download=False)
            return "inner_product"
        return eng.ctx.map_asym(R) if Rs is None else _ap_at(eng.ctx, Rs, True, asym=True)
    if mode == "rerank":
        if q_codes.shape[1] > 255:
            raise ValueError("inner-product ranking supports up to 255 features (have %d)" % q_codes.shape[1])
        if lists:
            eng.ctx.topr_rerank(R, download=False)
            return "rerank"
        return eng.ctx.map_rerank(R) if Rs is None else _ap_at(eng.ctx, Rs, False, rerank=True)
    qk, dk = _kind(eng.ctx, 1), eng.db_kind

    def hamming():
        if lists:
            eng.ctx.topr(R)
            return "hamming"
        return eng.average_precisions(R) if Rs is None else _ap_at(eng.ctx, Rs, False)

    if mode == "sign" or {qk, dk} <= {"pm1", "ones"}:
        return hamming()
    if mode == "codes":
        if {qk, dk} <= {"bits", "ones"}:
            return hamming()
        raise ValueError("codes must be binary -- all {0,1} or all {-1,+1}, the same spelling for queries and "
                         "database (found %s queries, %s database); binarise first (np.sign), or hand real-valued "
                         "features to MAPs.get_maps_by_feature, which ranks them by inner product like metric.py:13" % (qk, dk))
    if q_codes.shape[1] > 255:                        # (the loaders take up to 255 columns)
        raise ValueError("inner-product ranking supports up to 255 features (have %d)" % q_codes.shape[1])
    if not eng.ctx.census(0)[3]:             # a +-1 database whose floats stayed on the host: bring them over now
        src = eng.db_src
        if src is None:                      # (a device database in 'reference' mode keeps its floats from the start)
            raise ValueError("the resident database holds no float features: load it again")
        _load_database(eng, src[0], src[1], floats=1)
        _set_queries(eng, q_codes, q_labels)
    if lists:
        eng.ctx.topr_real(R, download=False)
        return "inner_product"
    if Rs is not None:
        return _ap_at(eng.ctx, Rs, True)
    return eng.ctx.map_real(R)


OUT_NAMES = ("idx", "dist", "score", "match", "ap", "hits")      # the results rank_into writes (keys of _native.OUT_ITEMS)


def _check_outs(outs, Q, N, R, stream):
    """rank_into's destinations, before any GPU use: {name: DeviceOut} of the ones given, each [Q, k] with 1 <= k <= R ([Q, 1] for
    "ap" and "hits"; a 1-D [Q] array counts as that)."""
    if not 1 <= R <= N:
        raise ValueError("R=%d must be in 1..N (N=%d database rows)" % (R, N))
    got = {}
    for name in OUT_NAMES:
        if outs.get(name) is None:
            continue
        d = as_device_output(outs[name], stream)
        per_query = name in ("ap", "hits")
        if d.shape[0] != Q or (d.shape[1] != 1 if per_query else not 1 <= d.shape[1] <= R):
            raise ValueError("%s must be [Q, %s] with Q=%d%s (got %r)" % (name, "1" if per_query else "k", Q, "" if per_query else
                                                                          ", 1 <= k <= R=%d" % R, d.shape))
        got[name] = d
    if not got:
        raise ValueError("rank_into needs at least one destination (%s)" % ", ".join(OUT_NAMES))
    return got


def _rank_into(eng, q_codes, q_labels, R, mode, outs):
    """One ranking with lists at R, the match and AP stages the destinations need, one export -> {"by": ..., "R": R}."""
    by = _rank(eng, q_codes, q_labels, R, mode, lists=True)
    if by == "inner_product" and "dist" in outs:
        raise ValueError("dist: an inner-product ranking has no Hamming distances (score has the inner products)")
    if by == "hamming" and "score" in outs:
        raise ValueError("score: a plain Hamming ranking has no scores (dist has the distances; MAPs(R, rerank=True) ranks with both)")
    if {"match", "ap", "hits"} & set(outs):
        eng.ctx.match()
    if {"ap", "hits"} & set(outs):
        eng.ctx.ap()
    eng.ctx.export([(name, d) for name, d in outs.items()])
    return {"by": by, "R": R}


def _evaluate(q_codes, db_codes, q_labels, db_labels, R, device, mode):
    db_codes, db_labels = _sides(db_codes, db_labels, "database")
    q_codes, q_labels = _sides(q_codes, q_labels, "query")
    _check_shapes(q_codes, db_codes, q_labels, db_labels, R)
    db_on_device = isinstance(db_codes, DeviceArray)
    eng = _Shared.get(device)
    with eng.lock:
        # the same read-only arrays as the last call (an evaluation loop over one database): the packed copy on the GPU
        # is still theirs -- skip pack + upload, like MAPs does (a writable array may have changed in place: reload)
        # (every load goes through _load_database, which clears `resident`: another database loaded into this shared
        # engine in between -- extra_metrics -- can never be mistaken for this one)
        res = eng.resident
        # (never for device arrays: nothing says their memory is unchanged -- residency comes from MAPs.set_database)
        same = (not db_on_device and res is not None and res[0] is db_codes and res[1] is db_labels and res[2] == mode
                and eng.db_src is not None and eng.db_src[0] is db_codes and eng.db_src[1] is db_labels
                and not db_codes.flags.writeable and not db_labels.flags.writeable)
        if not same:
            eng.resident = None
            _load_database(eng, db_codes, db_labels, mode)
            eng.resident = None if db_on_device else (db_codes, db_labels, mode)
        try:
            ap, rel = _rank(eng, q_codes, q_labels, R, mode)
        except Exception:
            eng.resident = None
            raise
    return mean_over_hits(ap, rel), ap, rel


# ------------------------------------------------------------------ reference surface
class MAPs:
    """Same constructor and method as lib/metric.py:4-24.

    The object holds one GPU context from first use to close() / garbage collection -- borrowed from a process-wide pool
    (_Pool: main.py:164 builds a new MAPs per evaluation, and a context of its own each time would cost allocations worth
    many times the evaluation) -- and a lock, so several live MAPs objects -- different R, different threads -- never share
    device state.  main.py:237-240 evaluates
    the same database against fresh queries again and again; `set_database` keeps it packed on the GPU between
    calls (explicit), and a database whose arrays are the SAME read-only objects as last time is reused
    automatically (a writable array may have changed in place, so it is uploaded again)."""

    def __init__(self, r, device=0, binarize=False, rerank=False, asymmetric=False, quantised=False, quantise_queries=False):
        """rerank=True: sign() first (it implies binarize), rank by Hamming distance, and inside equal distances by the float32 inner
        product of the features (descending), then by database index -- the ties of the Hamming ranking resolved by the
        magnitudes sign() throws away; the threshold group's rows with the highest inner product make the cut at R.
        asymmetric=True: what a deployed hashing system ranks -- the database is its sign() codes (bit = feature > 0, read as +-1; its
        floats never go to the GPU), the query keeps its float32 features, rows are ranked by their inner product (descending), then by
        database index (hg_map_asym).  Not together with binarize or rerank (ValueError).
        quantised=True: the database is product-quantisation codes (hashgan_amd/pq.py) -- `database` exposes .codes uint8 [N, M],
        .codebooks float32 [M, K, dsub] and .label, host arrays -- and rows are ranked by the float32 inner product of the query with
        the decoded row (descending), then by database index (hg_map_pq): AQD.  `query` exposes .output [Q, M * dsub], or, without an
        .output, .codes uint8 [Q, M], decoded on the host with the database's codebooks: SQD.  The decoded database exists nowhere.
        Not together with binarize, rerank or asymmetric (ValueError).  A database that exposes .output (host or device memory) and
        .codebooks and no .codes is encoded on the GPU on its way in (hg_set_database_pq_f32 / hg_pq_encode_dev: the exact encoder).
        quantise_queries=True (with quantised=True only): the query's .output is encoded on the GPU with the resident codebooks and
        decoded on the host -- SQD from features."""
        if quantise_queries and not quantised:
            raise ValueError("quantise_queries=True quantises the query with the database's codebooks: only together with quantised=True")
        if quantised and (binarize or rerank or asymmetric):
            raise ValueError("quantised=True ranks real-valued queries against product-quantisation codes: not together with binarize, "
                             "rerank or asymmetric")
        if asymmetric and (binarize or rerank):
            raise ValueError("asymmetric=True ranks real-valued queries against sign() codes: not together with binarize or rerank")
        self.R = r
        self.device = device
        self.binarize = binarize or rerank
        self.rerank = rerank
        self.asymmetric = asymmetric
        self.quantised = quantised
        self.quantise_queries = quantise_queries
        self._books = None             # quantised: the resident database's codebooks (a query given as codes is decoded with them)
        self._eng = None
        self._lock = threading.RLock()
        self._resident = None          # (output array, label array) the engine holds, or ("explicit",)

    # lib/metric.py:8-10 (unused by the reference; kept for surface parity)
    @staticmethod
    def distance(a, b):
        return np.dot(a, b)

    def _engine(self):
        if self._eng is None:
            self._eng = _Pool.acquire(self.device)
        return self._eng

    def _mode(self):
        return "quantised" if self.quantised else "asymmetric" if self.asymmetric else "rerank" if self.rerank else "sign" if self.binarize else "reference"

    def _db_sides(self, database):
        """database -> (features, labels) as the loaders take them; quantised: (PQTable of .codes / .codebooks, labels)."""
        if not self.quantised:
            return _sides(database.output, database.label, "database")
        books = getattr(database, "codebooks", None)
        if books is None or (getattr(database, "codes", None) is None and getattr(database, "output", None) is None):
            raise ValueError("quantised=True ranks a database given as .codes / .codebooks (hashgan_amd/pq.py), not as .output")
        if as_device_array(database.label) is not None:
            raise ValueError("quantised=True takes the database as host arrays")
        if getattr(database, "codes", None) is None:   # .output + .codebooks: encoded on the GPU
            return PQFeatures(database.output, books), np.asarray(database.label)
        return PQTable(database.codes, books), np.asarray(database.label)

    def _q_sides(self, database, query):
        """query -> (features, labels); quantised and no .output: its .codes decoded with the database's codebooks (SQD)."""
        if not self.quantised or (getattr(query, "output", None) is not None and not self.quantise_queries):
            return _sides(query.output, query.label, "query")
        from . import pq
        books = self._books if database is None else database.codebooks
        if books is None:
            raise ValueError("no resident database: call set_database first")
        if not self.quantise_queries:
            return pq.decode(query.codes, books), np.asarray(query.label)
        # SQD from features: the query's codes from the GPU's encoder (it leaves the context's tables alone), decoded on the host
        if getattr(query, "output", None) is None:
            raise ValueError("quantise_queries=True quantises query.output: the query has none")
        if as_device_array(query.label) is not None:
            raise ValueError("quantise_queries=True takes the query's labels as a host array")
        feats = PQFeatures(query.output, books)       # (shape and dtype checked before any GPU use)
        with self._lock:
            codes, _, bad_rows = self._guard(self._engine().ctx.pq_encode, feats.features, feats.codebooks)
        if bad_rows:
            raise ValueError("%d query rows are not finite" % bad_rows)
        return pq.decode(codes, feats.codebooks), np.asarray(query.label)

    def close(self):
        with self._lock:
            if self._eng is not None:
                eng, self._eng = self._eng, None
                self._resident = None
                _Pool.release(eng)

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass

    def set_database(self, database):
        """Upload + pack `database` (.output [N, b], .label [N, C]) once; get_maps_by_feature(None, query) -- or with
        the same object -- then ranks against the resident copy.  Arrays in device memory are copied in: the caller may
        overwrite them afterwards."""
        out, lab = self._db_sides(database)
        if out.ndim != 2 or lab.ndim != 2 or out.shape[0] != lab.shape[0]:
            raise ValueError("database.output must be [N, b] and database.label [N, C]")
        with self._lock:
            self._resident = None                      # a failed load leaves NO database (never the previous one half replaced)
            self._guard(_load_database, self._engine(), out, lab, self._mode())
            self._resident = ("explicit", database)
            self._books = out.codebooks if self.quantised else None

    def _guard(self, fn, *args):
        """A HIP-level failure (a fault, out of memory) may leave the context unusable: it is destroyed, not recycled."""
        try:
            return fn(*args)
        except _native.HashganNativeError as e:
            if e.code in (_native.HG_ERR_HIP, _native.HG_ERR_NOMEM) and self._eng is not None:
                self._eng.poisoned = True
            raise

    def _ensure_database(self, database):
        if database is None:
            if self._resident is None:
                raise ValueError("no resident database: call set_database first")
            return
        if self._resident is not None and self._resident[0] == "explicit" and self._resident[1] is database:
            return
        out, lab = self._db_sides(database)
        # device arrays handed over here are loaded on every call (nothing says their memory is unchanged).  What the load leaves is
        # the library's own copy, so a later get_maps_by_feature(None, query) ranks against it like after set_database.
        on_device = isinstance(out, DeviceArray)
        if self.quantised:
            if (self._resident is not None and self._resident[0] == "auto" and out.same_readonly(self._resident[1])
                    and self._resident[2] is lab and not lab.flags.writeable):
                return
        elif (not on_device and self._resident is not None and self._resident[0] == "auto" and self._resident[1] is out
                and self._resident[2] is lab and not out.flags.writeable and not lab.flags.writeable):
            return                                     # the very same immutable arrays as last time
        if out.ndim != 2 or lab.ndim != 2 or out.shape[0] != lab.shape[0]:
            raise ValueError("database.output must be [N, b] and database.label [N, C]")
        self._resident = None                          # a failed load leaves NO database
        self._guard(_load_database, self._engine(), out, lab, self._mode())
        self._resident = ("device",) if on_device else ("auto", out, lab)
        self._books = out.codebooks if self.quantised else None

    def get_maps_by_feature(self, database, query):
        """database/query: objects with .output [n, b] and .label [n, C] (main.py:157); database first."""
        q_codes, q_labels = self._q_sides(database, query)
        with self._lock:
            self._ensure_database(database)
            eng = self._engine()
            if eng.b is None:
                self._resident = None
                raise ValueError("no resident database: the last load failed")
            if q_codes.ndim != 2 or q_codes.shape[1] != eng.b:
                raise ValueError("query and database codes must be [n, b] with the same b")
            if q_labels.ndim != 2 or q_labels.shape[1] != eng.C or q_labels.shape[0] != q_codes.shape[0]:
                raise ValueError("query labels must be [Q, C] with the database's C")
            R = int(self.R)
            if not 1 <= R <= eng.N:
                raise ValueError("R=%d must be in 1..N (N=%d database rows)" % (R, eng.N))
            ap, rel = self._guard(_rank, eng, q_codes, q_labels, R, self._mode())
        return mean_over_hits(ap, rel)


    def get_maps_at(self, database, query, Rs):
        """mAP@R for every R of the strictly ascending cut-offs Rs (at most 64, each in 1..N) from ONE ranking at Rs[-1]: the top R is
        a prefix of the top Rs[-1], and each entry has the bits MAPs(R).get_maps_by_feature(database, query) returns.  Database
        residency, `binarize` and the routing (+-1 codes by Hamming distance, anything else by inner product) are
        get_maps_by_feature's; self.R is not used.  -> float64 [len(Rs)]"""
        q_codes, q_labels = self._q_sides(database, query)
        Rs = _check_cutoffs(Rs, None)
        if q_codes.ndim != 2 or q_labels.ndim != 2 or q_labels.shape[0] != q_codes.shape[0]:
            raise ValueError("query.output must be [Q, b] and query.label [Q, C]")
        if database is not None:                       # (what can be refused before any GPU use is)
            out, lab = self._db_sides(database)
            if out.ndim != 2 or lab.ndim != 2 or out.shape[0] != lab.shape[0]:
                raise ValueError("database.output must be [N, b] and database.label [N, C]")
            if q_codes.shape[1] != out.shape[1]:
                raise ValueError("query and database codes must be [n, b] with the same b")
            if q_labels.shape[1] != lab.shape[1]:
                raise ValueError("query labels must be [Q, C] with the database's C")
            if Rs[-1] > out.shape[0]:
                raise ValueError("R=%d must be in 1..N (N=%d database rows)" % (Rs[-1], out.shape[0]))
        with self._lock:
            self._ensure_database(database)
            eng = self._engine()
            if eng.b is None:
                self._resident = None
                raise ValueError("no resident database: the last load failed")
            if q_codes.shape[1] != eng.b:
                raise ValueError("query and database codes must be [n, b] with the same b")
            if q_labels.shape[1] != eng.C:
                raise ValueError("query labels must be [Q, C] with the database's C")
            if Rs[-1] > eng.N:
                raise ValueError("R=%d must be in 1..N (N=%d database rows)" % (Rs[-1], eng.N))
            ap, rel = self._guard(_rank, eng, q_codes, q_labels, int(Rs[-1]), self._mode(), Rs)
        out = np.empty(len(Rs), dtype=np.float64)
        for j in range(len(Rs)):
            out[j] = mean_over_hits(np.ascontiguousarray(ap[:, j]), np.ascontiguousarray(rel[:, j]))
        return out

    def get_knn_at(self, database, query, ks):
        """k-nearest-neighbour accuracy by majority vote of the retrieved labels and the retrieval confusion matrix at the strictly
        ascending cut-offs ks (at most 64, each in 1..N; up to 255 classes) from ONE ranking with lists at ks[-1] (hg_votes walks the
        lists; the list-free ranking get_maps_by_feature uses leaves nothing to vote on).  Database residency, `binarize`, `rerank` and
        the routing are get_maps_at's; self.R is not used.  -> extra_metrics.knn_from_tables' dict"""
        from . import extra_metrics as X               # (extra_metrics imports this module)
        q_codes, q_labels = self._q_sides(database, query)
        ks = _check_cutoffs(ks, None, "ks")
        if q_codes.ndim != 2 or q_labels.ndim != 2 or q_labels.shape[0] != q_codes.shape[0]:
            raise ValueError("query.output must be [Q, b] and query.label [Q, C]")
        if q_labels.shape[1] > X.MAX_CLASSES:
            raise ValueError("class votes take up to %d classes (have %d)" % (X.MAX_CLASSES, q_labels.shape[1]))
        if database is not None:                       # (what can be refused before any GPU use is)
            out, lab = self._db_sides(database)
            if out.ndim != 2 or lab.ndim != 2 or out.shape[0] != lab.shape[0]:
                raise ValueError("database.output must be [N, b] and database.label [N, C]")
            if q_codes.shape[1] != out.shape[1]:
                raise ValueError("query and database codes must be [n, b] with the same b")
            if q_labels.shape[1] != lab.shape[1]:
                raise ValueError("query labels must be [Q, C] with the database's C")
            if ks[-1] > out.shape[0]:
                raise ValueError("k=%d must be in 1..N (N=%d database rows)" % (ks[-1], out.shape[0]))
        with self._lock:
            self._ensure_database(database)
            eng = self._engine()
            if eng.b is None:
                self._resident = None
                raise ValueError("no resident database: the last load failed")
            if q_codes.shape[1] != eng.b:
                raise ValueError("query and database codes must be [n, b] with the same b")
            if q_labels.shape[1] != eng.C:
                raise ValueError("query labels must be [Q, C] with the database's C")
            if ks[-1] > eng.N:
                raise ValueError("k=%d must be in 1..N (N=%d database rows)" % (ks[-1], eng.N))
            self._guard(_rank, eng, q_codes, q_labels, int(ks[-1]), self._mode(), None, True)
            pred, conf = self._guard(X._vote_tables, eng.ctx, ks)
            words = eng.ctx.get_packed(1)[1]           # the queries' labels as the GPU holds them (device arrays never come to the host otherwise)
        lab = (words[:, np.arange(eng.C) // 64] >> (np.arange(eng.C) % 64).astype(np.uint64)) & np.uint64(1)
        return X.knn_from_tables(pred, conf, lab, ks)

    def rank_into(self, database, query, idx=None, dist=None, score=None, match=None, ap=None, hits=None, stream=None):
        """Rank `query` against `database` at self.R and write the results into arrays of the caller's in GPU memory -- no host pass:
        idx [Q, k] int64 | int32 ranked database indices, dist [Q, k] uint8 | int32 Hamming distances, score [Q, k] float32 inner
        products, match [Q, k] uint8 / bool label match per rank, ap [Q] or [Q, 1] float64 | float32 (nan: no hit in the top R), hits
        [Q] or [Q, 1] int64 | int32; k <= R gives the first k ranks.  Destinations: torch tensors on the device, anything with
        __cuda_array_interface__, devarray.DeviceOut (devarray.as_device_output); `stream` is the consumer's HIP stream (an int
        handle, e.g. torch.cuda.current_stream().cuda_stream): what it holds so far is waited for, what is enqueued on it afterwards
        sees the data.  Database residency, `binarize`, `rerank` and the routing are get_maps_by_feature's.  dist on an inner-product
        ranking and score on a plain Hamming ranking raise ValueError.  -> {"by": "hamming" | "inner_product" | "rerank", "R": R}"""
        q_codes, q_labels = self._q_sides(database, query)
        if q_codes.ndim != 2 or q_labels.ndim != 2 or q_labels.shape[0] != q_codes.shape[0]:
            raise ValueError("query.output must be [Q, b] and query.label [Q, C]")
        R = int(self.R)
        given = dict(idx=idx, dist=dist, score=score, match=match, ap=ap, hits=hits)
        if database is not None:                       # (what can be refused before any GPU use is)
            out, lab = self._db_sides(database)
            _check_shapes(q_codes, out, q_labels, lab, R)
            outs = _check_outs(given, q_codes.shape[0], out.shape[0], R, stream)
        with self._lock:
            self._ensure_database(database)
            eng = self._engine()
            if eng.b is None:
                self._resident = None
                raise ValueError("no resident database: the last load failed")
            if q_codes.shape[1] != eng.b:
                raise ValueError("query and database codes must be [n, b] with the same b")
            if q_labels.shape[1] != eng.C:
                raise ValueError("query labels must be [Q, C] with the database's C")
            outs = _check_outs(given, q_codes.shape[0], eng.N, R, stream)
            return self._guard(_rank_into, eng, q_codes, q_labels, R, self._mode(), outs)


def MAP(query_codes, db_codes, query_labels, db_labels, R, device=0):
    """mAP@R of binary codes, query-first argument order (BASELINE.json north star).  Codes must be binary --
    {0,1} bits or +-1, ranked by Hamming distance; real-valued features belong to MAPs.get_maps_by_feature."""
    return _evaluate(query_codes, db_codes, query_labels, db_labels, int(R), device, "codes")[0]


calc_map = MAP


def MAP_per_query(query_codes, db_codes, query_labels, db_labels, R, device=0):
    """(mAP, ap [Q] with nan for skipped queries, rel [Q]); binary codes like MAP."""
    return _evaluate(query_codes, db_codes, query_labels, db_labels, int(R), device, "codes")
