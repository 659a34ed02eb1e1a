"""ctypes binding of libhashgan_amd.so (the C ABI in include/hashgan_amd.h).

There is no CPU implementation behind this module: if the library is missing,
fails to load, or finds no GPU, the error propagates (HashganNativeError).
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

HG_OK, HG_ERR_ARG, HG_ERR_HIP, HG_ERR_STATE, HG_ERR_NOMEM = 0, -1, -2, -3, -4
IDX_NONE = 0xFFFFFFFF
COMM_ID_BYTES = 128


class HashganNativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hashgan_amd native error %d: %s" % (code, msg))
        self.code = code


_p = C.c_void_p
_i64 = C.c_int64
# name -> (argtypes); every function returns int except hg_last_error
_SIGNATURES = {
    "hg_version": [],
    "hg_device_count": [C.POINTER(C.c_int)],
    "hg_init": [C.c_int, C.POINTER(_p)],
    "hg_destroy": [_p],
    "hg_pack_sign_f32": [_p, _i64, C.c_int, _p],
    "hg_set_database": [_p, _p, _p, _i64, C.c_int, C.c_int, _i64, _i64],
    "hg_set_queries": [_p, _p, _p, _i64],
    "hg_set_database_f32": [_p, _p, _p, _i64, C.c_int, C.c_int, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64)],
    "hg_set_queries_f32": [_p, _p, _p, _i64, C.POINTER(_i64), C.POINTER(_i64)],
    "hg_set_database_dev": [_p, _p, _p, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64)],
    "hg_set_queries_dev": [_p, _p, _p, C.POINTER(_i64), C.POINTER(_i64)],
    "hg_export": [_p, _p, C.c_int],
    "hg_get_packed": [_p, C.c_int, _p, _p],
    "hg_hist": [_p],
    "hg_hist_buffer": [_p, C.POINTER(_p), C.POINTER(_i64)],
    "hg_rel_hist": [_p],
    "hg_grade_hist": [_p],
    "hg_joint_hist": [_p],
    "hg_graded": [_p, _p, C.c_int, _p, _p, C.c_int],
    "hg_tie_ap": [_p, _p, C.c_int],
    "hg_ap_at": [_p, _p, C.c_int],
    "hg_votes": [_p, _p, C.c_int],
    "hg_plan": [_p, _i64, _p, C.c_int, C.c_int],
    "hg_select": [_p],
    "hg_bet_eligible": [_p, _i64, C.c_int, C.POINTER(C.c_int)],
    "hg_sample_hist": [_p, _i64],
    "hg_guess": [_p, _i64, _p, C.c_int, C.c_int],
    "hg_select_candidates": [_p],
    "hg_rank": [_p, _p, C.c_int, C.c_int, C.POINTER(C.c_int)],
    "hg_bet_verdict": [_p, C.POINTER(C.c_int)],
    "hg_select_ranked": [_p],
    "hg_merge_ranked": [_p, _p, _p, C.c_int, C.POINTER(C.c_int)],
    "hg_merge_ap_part": [_p, _p, _p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.POINTER(_p), C.POINTER(C.c_int64)],
    "hg_unpack_parts": [_p, _p, C.c_int, C.c_int64, _p, _p, C.POINTER(C.c_int)],
    "hg_pack_sample_by_owner": [_p, C.c_int, C.POINTER(_p), C.POINTER(C.c_int64)],
    "hg_guess_owned": [_p, _i64, _p, C.c_int, C.c_int, C.POINTER(_p), C.POINTER(C.c_int64)],
    "hg_guess_finish": [_p, _i64, _p, C.c_int, C.c_int],
    "hg_pack_ranked_by_owner": [_p, C.c_int, C.POINTER(_p), C.POINTER(C.c_int64)],
    "hg_merge_ap_owned": [_p, _p, C.c_int, C.c_int, C.POINTER(_p), C.POINTER(C.c_int64)],
    "hg_match": [_p],
    "hg_match_buffer": [_p, C.POINTER(_p), C.POINTER(_i64)],
    "hg_merge_match": [_p, _p, C.c_int],
    "hg_ap": [_p],
    "hg_topr_buffers": [_p, C.POINTER(_p), C.POINTER(_p), C.POINTER(_i64)],
    "hg_merge_topr": [_p, _p, _p, C.c_int],
    "hg_topr": [_p, _i64],
    "hg_map": [_p, _i64, _p, _p],
    "hg_map_begin": [_p, _i64],
    "hg_map_end": [_p, _p, _p],
    "hg_map_real": [_p, _i64, _p, _p],
    "hg_topr_real": [_p, _i64],
    "hg_get_topr_real": [_p, _p, _p],
    "hg_map_asym": [_p, _i64, _p, _p],
    "hg_topr_asym": [_p, _i64],
    "hg_set_database_pq": [_p, _p, _p, _p, _i64, C.c_int, C.c_int, C.c_int, C.c_int, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64)],
    "hg_map_pq": [_p, _i64, _p, _p],
    "hg_topr_pq": [_p, _i64],
    "hg_pq_encode": [_p, _p, _i64, _p, C.c_int, C.c_int, C.c_int, _p, _p, C.POINTER(_i64)],
    "hg_pq_encode_dev": [_p, _p, _p, C.c_int, C.c_int, C.c_int, _p, _p, C.POINTER(_i64)],
    "hg_set_database_pq_f32": [_p, _p, _p, _p, _i64, C.c_int, C.c_int, C.c_int, C.c_int, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64),
                               C.POINTER(_i64)],
    "hg_topr_rerank": [_p, _i64],
    "hg_map_rerank": [_p, _i64, _p, _p],
    "hg_get_rerank_scores": [_p, _p],
    "hg_get_topr": [_p, _p, _p],
    "hg_get_match": [_p, _p],
    "hg_get_ap": [_p, _p, _p],
    "hg_get_hist": [_p, _p],
    "hg_get_rel_hist": [_p, _p, _p],
    "hg_get_grade_hist": [_p, _p],
    "hg_get_joint_hist": [_p, _p],
    "hg_get_graded": [_p, _p, _p, _p, _p],
    "hg_get_grades": [_p, _p],
    "hg_pack_side_table": [_p, C.c_int, C.c_int, C.POINTER(_p), C.POINTER(_i64)],
    "hg_merge_side_table": [_p, C.c_int, _p, C.c_int, C.c_int],
    "hg_pack_list_table": [_p, C.c_int, _p, C.c_int, C.POINTER(_p), C.POINTER(_i64)],
    "hg_merge_list_table": [_p, C.c_int, _p, C.c_int, _p, C.c_int],
    "hg_get_merged_rel_hist": [_p, _p, _p],
    "hg_get_merged_grade_hist": [_p, _p],
    "hg_get_merged_joint_hist": [_p, _p],
    "hg_get_tie_ap": [_p, _p, _p, _p, _p, _p, _p, _p],
    "hg_get_ap_at": [_p, _p, _p],
    "hg_get_vote_pred": [_p, _p, _p],
    "hg_get_vote_confusion": [_p, _p],
    "hg_get_votes": [_p, _p],
    "hg_set_neighbours": [_p, _p, _i64, C.c_int],
    "hg_neighbours_from_lists": [_p, C.c_int],
    "hg_get_neighbours": [_p, _p, _p],
    "hg_match_neighbours": [_p],
    "hg_nbr_hist": [_p],
    "hg_get_nbr_hist": [_p, _p, _p],
    "hg_comm_unique_id": [_p],
    "hg_comm_init": [_p, _p, C.c_int, C.c_int],
    "hg_comm_destroy": [_p],
    "hg_comm_info": [_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "hg_allgather": [_p, C.c_int, _p, _i64, C.POINTER(_p)],
    "hg_alltoall": [_p, C.c_int, _p, _i64, C.POINTER(_p)],
    "hg_allgather_topr": [_p],
    "hg_allreduce_max_f64": [_p, C.POINTER(C.c_double)],
    "hg_barrier": [_p],
    "hg_scratch": [_p, C.c_int, _i64, C.POINTER(_p)],
    "hg_memcpy_dtod": [_p, _p, _p, _i64],
    "hg_memcpy_dtoh": [_p, _p, _p, _i64],
    "hg_memcpy_htod": [_p, _p, _p, _i64],
    "hg_synchronize": [_p],
    "hg_set_stream": [_p, _p],
    "hg_set_option": [_p, C.c_char_p, _i64],
    "hg_get_stat": [_p, C.c_char_p, C.POINTER(_i64)],
    "hg_get_census": [_p, C.c_int, C.POINTER(_i64)],
    "hg_shard_step": [_p, _i64, C.c_int, _p, _p, C.POINTER(C.c_int)],
    "hg_trim": [_p],
    "hg_release_cache": [],
    "hg_preload": [_p],
    "hg_timing_enable": [_p, C.c_int],
    "hg_timing_reset": [_p],
    "hg_timing_read": [_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(_i64), C.POINTER(C.c_int)],
}
EXPORTS = sorted(list(_SIGNATURES) + ["hg_last_error"])

_lib = None

# hg_dev_array.dtype (include/hashgan_amd.h)
HG_F32, HG_F16, HG_BF16, HG_I64, HG_I32, HG_U8, HG_F64 = range(7)      # (HG_F64: destinations of hg_export only; the loaders refuse it)
DEV_DTYPES = {"float32": HG_F32, "float16": HG_F16, "bfloat16": HG_BF16, "int64": HG_I64, "int32": HG_I32, "uint8": HG_U8, "bool": HG_U8,
              "float64": HG_F64}
# hg_export_item.what
HG_OUT_IDX, HG_OUT_DIST, HG_OUT_SCORE, HG_OUT_MATCH, HG_OUT_AP, HG_OUT_HITS, HG_OUT_GRADES = range(7)
OUT_ITEMS = {"idx": HG_OUT_IDX, "dist": HG_OUT_DIST, "score": HG_OUT_SCORE, "match": HG_OUT_MATCH, "ap": HG_OUT_AP, "hits": HG_OUT_HITS,
             "grades": HG_OUT_GRADES}
# hg_pack_side_table / hg_merge_side_table: which
HG_SIDE_REL, HG_SIDE_GRADE, HG_SIDE_JOINT = range(3)
SIDE_TABLES = {"rel": HG_SIDE_REL, "grade": HG_SIDE_GRADE, "joint": HG_SIDE_JOINT}
# hg_pack_list_table / hg_merge_list_table: which
HG_LIST_GRADES, HG_LIST_VOTES = range(2)
LIST_TABLES = {"grades": HG_LIST_GRADES, "votes": HG_LIST_VOTES}


class DevArrayStruct(C.Structure):
    """hg_dev_array: a 2-D array in device memory, strides in elements."""
    _fields_ = [("ptr", _p), ("rows", _i64), ("cols", _i64), ("row_stride", _i64), ("col_stride", _i64),
                ("dtype", C.c_int), ("stream", _p)]


class ExportItemStruct(C.Structure):
    """hg_export_item: what to write, and where."""
    _fields_ = [("what", C.c_int), ("dst", DevArrayStruct)]


def _dev_struct(a):
    """devarray.DeviceArray (or anything with ptr / shape / strides / dtype / stream) -> hg_dev_array.  An unknown dtype name goes
    down as -1: the library refuses it with HG_ERR_ARG like every other bad descriptor."""
    return DevArrayStruct(_p(int(a.ptr)), int(a.shape[0]), int(a.shape[1]), int(a.strides[0]), int(a.strides[1]),
                          DEV_DTYPES.get(str(a.dtype), -1), _p(int(a.stream)) if a.stream else None)


def library_path():
    """The production library, or the one HG_LIBRARY names (e.g. the probe build)."""
    return os.environ.get("HG_LIBRARY") or _build.LIB_PATH


def load():
    """dlopen the library (no GPU needed for this step) and bind every symbol."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise HashganNativeError(HG_ERR_STATE, "%s not built -- run `python -m hashgan_amd.build` "
                                 "(or __graft_entry__.build())" % path)
    lib = C.CDLL(path)
    for name, args in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.hg_last_error.argtypes = []
    lib.hg_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def check(rc):
    if rc != HG_OK:
        raise HashganNativeError(rc, load().hg_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return a.ctypes.data_as(_p) if a is not None else None


def _carray(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


def _labels_i64(labels):
    """Labels as the int64 matrix the C ABI takes.  The {0,1} census runs on the GPU AFTER this conversion, so a
    conversion that changes a value (0.5 -> 0, 1.7 -> 1) would let a matrix through that lib/metric.py:19's
    `database.label == label` never matches: such labels are refused here."""
    a = np.asarray(labels)
    out = _carray(a, np.int64)
    if a.dtype.kind not in "iub" and not np.array_equal(out, a):
        raise ValueError("labels must be {0,1} indicator matrices")
    return out


class Context:
    """One GPU context (hg_ctx).  Thin, 1:1 with the C ABI."""

    def __init__(self, device=0):
        self._lib = load()
        h = _p()
        check(self._lib.hg_init(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.Q = self.N = self.R = self.b = self.C = None
        self.n_total = None                # rows of the whole database the loaded one is a shard of (N unless set_database* said otherwise)
        self.options_touched = set()       # keys set through set_option (metric's engine pool only recycles contexts on their defaults)
        self.option_values = {}            # ... and the values they were last set to (the library has no getter)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs ---------------------------------------------------------------
    def set_database(self, codes_u64, labels_u64, b, C_, idx_base=0, n_total=None):
        codes = _carray(codes_u64, np.uint64)
        labels = _carray(labels_u64, np.uint64)
        N = codes.shape[0]
        n_total = N if n_total is None else int(n_total)
        check(self._lib.hg_set_database(self._h, _ptr(codes), _ptr(labels), N, int(b), int(C_), int(idx_base), n_total))
        self.N, self.b, self.C, self.n_total = N, int(b), int(C_), n_total

    def set_queries(self, codes_u64, labels_u64):
        codes = _carray(codes_u64, np.uint64)
        labels = _carray(labels_u64, np.uint64)
        check(self._lib.hg_set_queries(self._h, _ptr(codes), _ptr(labels), codes.shape[0]))
        self.Q = codes.shape[0]

    def set_database_f32(self, features, labels, idx_base=0, n_total=None):
        """float32 [N, b] features + int64 [N, C] labels; binarise + pack on the GPU.
        -> (entries outside {-1,0,+1}, label entries outside {0,1})"""
        x = _carray(features, np.float32)
        lab = _labels_i64(labels)
        N, b = x.shape
        n_total = N if n_total is None else int(n_total)
        bc, bl = _i64(), _i64()
        check(self._lib.hg_set_database_f32(self._h, _ptr(x), _ptr(lab), N, b, lab.shape[1], int(idx_base), n_total,
                                            C.byref(bc), C.byref(bl)))
        self.N, self.b, self.C, self.n_total = N, b, lab.shape[1], n_total
        return bc.value, bl.value

    def set_queries_f32(self, features, labels):
        x = _carray(features, np.float32)
        lab = _labels_i64(labels)
        bc, bl = _i64(), _i64()
        check(self._lib.hg_set_queries_f32(self._h, _ptr(x), _ptr(lab), x.shape[0], C.byref(bc), C.byref(bl)))
        self.Q = x.shape[0]
        return bc.value, bl.value

    def set_database_dev(self, features, labels, idx_base=0, n_total=None):
        """The same from arrays in DEVICE memory (devarray.DeviceArray: any strides; float32 / float16 / bfloat16 features, int64 /
        int32 / uint8 / float32 labels), packed by one kernel straight out of the caller's memory; complete -- the arrays free to be
        overwritten -- on return (hg_set_database_dev).  -> (entries outside {-1,0,+1}, label entries outside {0,1})"""
        f, l = _dev_struct(features), _dev_struct(labels)
        n_total = f.rows if n_total is None else int(n_total)
        bc, bl = _i64(), _i64()
        check(self._lib.hg_set_database_dev(self._h, C.byref(f), C.byref(l), int(idx_base), n_total, C.byref(bc), C.byref(bl)))
        self.N, self.b, self.C, self.n_total = f.rows, f.cols, l.cols, n_total
        return bc.value, bl.value

    def set_queries_dev(self, features, labels):
        """Queries from arrays in device memory, like set_database_dev (hg_set_queries_dev); same b and C as the database, their
        floats kept iff the database's are.  -> (entries outside {-1,0,+1}, label entries outside {0,1})"""
        f, l = _dev_struct(features), _dev_struct(labels)
        bc, bl = _i64(), _i64()
        check(self._lib.hg_set_queries_dev(self._h, C.byref(f), C.byref(l), C.byref(bc), C.byref(bl)))
        self.Q = f.rows
        return bc.value, bl.value

    def export(self, items):
        """Results into the caller's device memory (hg_export): items = [(what, destination), ...], what an HG_OUT_* value or a key of
        OUT_ITEMS ("idx", "dist", "score", "match", "ap", "hits", "grades"), destination a devarray.DeviceOut (or anything with ptr /
        shape / strides / dtype / stream) of shape [Q, k], k <= R -- [Q, 1] for "ap" and "hits" --, its stream the consumer's.  Every
        item is checked before anything is written; ordering and refusals: include/hashgan_amd.h."""
        items = list(items)
        arr = (ExportItemStruct * max(len(items), 1))()
        for i, (what, dst) in enumerate(items):
            arr[i].what = OUT_ITEMS[what] if isinstance(what, str) else int(what)
            arr[i].dst = _dev_struct(dst)
        check(self._lib.hg_export(self._h, arr, len(items)))

    def get_packed(self, which):
        n = self.Q if which else self.N
        codes = np.empty((n, (self.b + 31) // 32), dtype=np.uint32)
        labels = np.empty((n, (self.C + 63) // 64), dtype=np.uint64)
        check(self._lib.hg_get_packed(self._h, int(which), _ptr(codes), _ptr(labels)))
        return codes, labels

    # -- stages -----------------------------------------------------------------
    def hist(self):
        check(self._lib.hg_hist(self._h))

    def rel_hist(self):
        """One pass over the pairs: rows per (distance, query) and how many of them share a label with the query."""
        check(self._lib.hg_rel_hist(self._h))

    def grade_hist(self):
        """One pass over the label pairs: rows per (grade, query), grade = labels shared with the query."""
        check(self._lib.hg_grade_hist(self._h))

    def joint_hist(self):
        """One pass over the pairs: rows per (distance, grade, query), grade = labels shared with the query."""
        check(self._lib.hg_joint_hist(self._h))

    def graded(self, ks, gain, disc, keep_grades=False):
        """Graded sums along the ranked lists of the last topr() / topr_real() at the ascending cut-offs ks; gain [C+1] and
        disc [max(ks)] are float64 tables (disc[i-1] for rank i).  Results: get_graded(), get_grades()."""
        ks = _carray(ks, np.int64).ravel()
        gain = _carray(gain, np.float64).ravel()
        disc = _carray(disc, np.float64).ravel()
        if len(gain) != (self.C or 0) + 1 or (len(ks) and len(disc) < int(ks[-1])):
            raise ValueError("gain must have C + 1 entries and disc max(ks)")
        check(self._lib.hg_graded(self._h, _ptr(ks), len(ks), _ptr(gain), _ptr(disc), 1 if keep_grades else 0))
        self._graded_nk = len(ks)

    def tie_ap(self, Rs):
        """Tie-aware AP at the strictly ascending cut-offs Rs (1..N, at most 64) from the relevant-row histogram, which is
        computed first unless the tables of the loaded queries and database are there.  Results: get_tie_ap()."""
        Rs = _carray(Rs, np.int64).ravel()
        check(self._lib.hg_tie_ap(self._h, _ptr(Rs), len(Rs)))
        self._tie_nR = len(Rs)

    def ap_at(self, Rs):
        """AP@R and the hits among the top R at the strictly ascending cut-offs Rs (at most 64, each within 1..R of the last ranking),
        in one pass over the match bitmap that ranking left (topr, topr_real, map, map_real).  Results: get_ap_at()."""
        Rs = _carray(Rs, np.int64).ravel()
        check(self._lib.hg_ap_at(self._h, _ptr(Rs), len(Rs)))
        self._ap_at_nR = len(Rs)

    def votes(self, ks):
        """Class votes along the ranked lists of the last topr() / topr_real() / topr_rerank() at the strictly ascending cut-offs ks (at
        most 64, each within 1..R of that ranking): how many of the first k ranks carry each class, the majority class, and the
        confusion matrix over the queries' own labels.  Results: get_vote_pred(), get_vote_confusion(), get_votes()."""
        ks = _carray(ks, np.int64).ravel()
        check(self._lib.hg_votes(self._h, _ptr(ks), len(ks)))
        self._votes_nk = len(ks)

    # -- label-free relevance: neighbour sets ----------------------------------------
    def set_neighbours(self, ids):
        """The ground-truth neighbour sets (hg_set_neighbours): ids [Q, G], a row the set of one loaded query in any order, IDX_NONE
        (0xFFFFFFFF) or a negative value padding a shorter set; 1 <= G <= 16384.  Duplicates and ids >= n_total are refused."""
        a = np.asarray(ids)
        if a.ndim != 2:
            raise ValueError("ids must be [Q, G]")
        if a.dtype != np.uint32:
            a = np.where(np.asarray(a, dtype=np.int64) < 0, IDX_NONE, a).astype(np.uint32)
        a = _carray(a, np.uint32)
        check(self._lib.hg_set_neighbours(self._h, _ptr(a), a.shape[0], a.shape[1]))
        self._nbr_G = a.shape[1]

    def neighbours_from_lists(self, G):
        """The first G ranks of the ranked lists the last topr() / topr_real() / topr_asym() / topr_rerank() left on the device become
        the neighbour sets (hg_neighbours_from_lists); nothing crosses to the host."""
        check(self._lib.hg_neighbours_from_lists(self._h, int(G)))
        self._nbr_G = int(G)

    def get_neighbours(self, ids=True):
        """-> (ids uint32 [Q, G] ascending, IDX_NONE pads at the end; count uint32 [Q]).  ids=False: the counts alone (ids is None)."""
        ids = np.empty((self.Q or 0, getattr(self, "_nbr_G", 0)), dtype=np.uint32) if ids else None
        cnt = np.empty(self.Q or 0, dtype=np.uint32)
        check(self._lib.hg_get_neighbours(self._h, _ptr(ids), _ptr(cnt)))
        return ids, cnt

    def match_neighbours(self):
        """The match bitmap of the last ranking's lists from the neighbour sets instead of the labels (hg_match_neighbours); ap(),
        ap_at(), get_match() and export() then work on it.  The next ranking brings the label bits back."""
        check(self._lib.hg_match_neighbours(self._h))

    def nbr_hist(self):
        """Neighbours per (Hamming distance, query) (hg_nbr_hist).  Results: get_nbr_hist()."""
        check(self._lib.hg_nbr_hist(self._h))

    def get_nbr_hist(self):
        """-> (nbr uint32 [b+1, Q], count uint32 [Q]) (after nbr_hist())."""
        h = np.empty(((self.b or 0) + 1, self.Q or 0), dtype=np.uint32)
        cnt = np.empty(self.Q or 0, dtype=np.uint32)
        check(self._lib.hg_get_nbr_hist(self._h, _ptr(h), _ptr(cnt)))
        return h, cnt

    def hist_buffer(self):
        p, n = _p(), _i64()
        check(self._lib.hg_hist_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def plan(self, R, dev_hist_all=None, G=1, rank=0):
        check(self._lib.hg_plan(self._h, int(R), _p(dev_hist_all) if dev_hist_all else None, int(G), int(rank)))
        self.R = int(R)

    def select(self):
        check(self._lib.hg_select(self._h))

    def bet_eligible(self, R, world=1):
        v = C.c_int()
        check(self._lib.hg_bet_eligible(self._h, int(R), int(world), C.byref(v)))
        return bool(v.value)

    def sample_hist(self, R):
        check(self._lib.hg_sample_hist(self._h, int(R)))

    def guess(self, R, dev_hist_all=None, G=1, rank=0):
        check(self._lib.hg_guess(self._h, int(R), _p(dev_hist_all) if dev_hist_all else None, int(G), int(rank)))
        self.R = int(R)

    def select_candidates(self):
        check(self._lib.hg_select_candidates(self._h))

    def rank(self, dev_hist_all=None, G=1, rank=0):
        lost = C.c_int()
        check(self._lib.hg_rank(self._h, _p(dev_hist_all) if dev_hist_all else None, int(G), int(rank), C.byref(lost)))
        return None if lost.value < 0 else bool(lost.value)      # None: verdict deferred (option defer_verdict)

    def select_ranked(self):
        check(self._lib.hg_select_ranked(self._h))

    def merge_ranked(self, dev_hist_all=None, dev_bits_all=None, G=1):
        lost = C.c_int()
        check(self._lib.hg_merge_ranked(self._h, _p(dev_hist_all) if dev_hist_all else None,
                                        _p(dev_bits_all) if dev_bits_all else None, int(G), C.byref(lost)))
        return None if lost.value < 0 else bool(lost.value)

    def merge_ap_part(self, dev_hist_all, dev_bits_all, G, q0, nq, width):
        """-> (device address, bytes) of this rank's part: hg_merge_ap_part."""
        p, n = _p(), _i64()
        check(self._lib.hg_merge_ap_part(self._h, _p(dev_hist_all) if dev_hist_all else None, _p(dev_bits_all) if dev_bits_all else None,
                                         int(G), int(q0), int(nq), int(width), C.byref(p), C.byref(n)))
        return p.value, n.value

    def unpack_parts(self, dev_parts_all, G, width):
        """-> (ap [Q] float64, rel [Q] int64, bet lost?) from the gathered parts: hg_unpack_parts."""
        ap = np.empty(self.Q, dtype=np.float64)
        rel = np.empty(self.Q, dtype=np.int64)
        lost = C.c_int()
        check(self._lib.hg_unpack_parts(self._h, _p(dev_parts_all), int(G), int(width), _ptr(ap), _ptr(rel), C.byref(lost)))
        return ap, rel, bool(lost.value)

    # -- the same bet with its exchanges routed by query owner (hg_pack_sample_by_owner ... hg_merge_ap_owned)
    def pack_sample_by_owner(self, G):
        p, n = _p(), _i64()
        check(self._lib.hg_pack_sample_by_owner(self._h, int(G), C.byref(p), C.byref(n)))
        return p.value, n.value                      # (device address of [G] blocks, bytes per block)

    def guess_owned(self, R, dev_recv, G, rank):
        p, n = _p(), _i64()
        check(self._lib.hg_guess_owned(self._h, int(R), _p(dev_recv), int(G), int(rank), C.byref(p), C.byref(n)))
        return p.value, n.value

    def guess_finish(self, R, dev_answers, G, rank):
        check(self._lib.hg_guess_finish(self._h, int(R), _p(dev_answers), int(G), int(rank)))
        self.R = int(R)

    def pack_ranked_by_owner(self, G):
        p, n = _p(), _i64()
        check(self._lib.hg_pack_ranked_by_owner(self._h, int(G), C.byref(p), C.byref(n)))
        return p.value, n.value

    def merge_ap_owned(self, dev_recv, G, rank):
        p, n = _p(), _i64()
        check(self._lib.hg_merge_ap_owned(self._h, _p(dev_recv), int(G), int(rank), C.byref(p), C.byref(n)))
        return p.value, n.value

    def bet_verdict(self):
        lost = C.c_int()
        check(self._lib.hg_bet_verdict(self._h, C.byref(lost)))
        return bool(lost.value)

    def match(self):
        check(self._lib.hg_match(self._h))

    def match_buffer(self):
        p, n = _p(), _i64()
        check(self._lib.hg_match_buffer(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def merge_match(self, dev_bits_all, G):
        check(self._lib.hg_merge_match(self._h, _p(dev_bits_all), int(G)))

    def ap(self):
        check(self._lib.hg_ap(self._h))

    def topr_buffers(self):
        a, b, n = _p(), _p(), _i64()
        check(self._lib.hg_topr_buffers(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def merge_topr(self, dev_idx_all, dev_dist_all, G):
        check(self._lib.hg_merge_topr(self._h, _p(dev_idx_all), _p(dev_dist_all), int(G)))

    # -- one-shot ---------------------------------------------------------------
    def topr(self, R):
        check(self._lib.hg_topr(self._h, int(R)))
        self.R = int(R)

    def map(self, R):
        ap = np.empty(self.Q, dtype=np.float64)
        rel = np.empty(self.Q, dtype=np.int64)
        check(self._lib.hg_map(self._h, int(R), _ptr(ap), _ptr(rel)))
        self.R = int(R)
        return ap, rel

    def map_begin(self, R):
        """First half of map(): enqueue a step and return (at most two in flight; see hg_map_begin in include/hashgan_amd.h)."""
        check(self._lib.hg_map_begin(self._h, int(R)))
        self.R = int(R)
        self._in_flight = getattr(self, "_in_flight", []) + [self.Q]      # (a step's results have the length of ITS query table)

    def map_end(self):
        """Second half of map(): wait for the oldest step in flight, return its (ap, rel)."""
        pending = getattr(self, "_in_flight", [])
        nq = pending[0] if pending else self.Q
        ap = np.empty(nq, dtype=np.float64)
        rel = np.empty(nq, dtype=np.int64)
        rc = self._lib.hg_map_end(self._h, _ptr(ap), _ptr(rel))
        self._in_flight = pending[1:]                    # (hg_map_end takes the step off its queue whatever it returns)
        check(rc)
        return ap, rel

    # -- real-valued features ---------------------------------------------------
    def map_real(self, R):
        ap = np.empty(self.Q, dtype=np.float64)
        rel = np.empty(self.Q, dtype=np.int64)
        check(self._lib.hg_map_real(self._h, int(R), _ptr(ap), _ptr(rel)))
        self.R = int(R)
        return ap, rel

    def topr_real(self, R, download=True):
        """download=False: the lists stay on the device (for graded())."""
        check(self._lib.hg_topr_real(self._h, int(R)))
        self.R = int(R)
        if not download:
            return None
        idx = np.empty((self.Q, self.R), dtype=np.uint32)
        score = np.empty((self.Q, self.R), dtype=np.float32)
        check(self._lib.hg_get_topr_real(self._h, _ptr(idx), _ptr(score)))
        return idx, score

    # -- asymmetric ranking: real-valued queries against the database's codes read as +-1 ------
    def map_asym(self, R):
        """(ap, rel) of hg_map_asym: needs the queries loaded under set_option("keep_query_floats", 1); any database loader."""
        ap = np.empty(self.Q, dtype=np.float64)
        rel = np.empty(self.Q, dtype=np.int64)
        check(self._lib.hg_map_asym(self._h, int(R), _ptr(ap), _ptr(rel)))
        self.R = int(R)
        return ap, rel

    def topr_asym(self, R, download=True):
        """-> (idx, score) of hg_topr_asym through hg_get_topr_real; download=False: the lists stay on the device (graded(), votes(), export())."""
        check(self._lib.hg_topr_asym(self._h, int(R)))
        self.R = int(R)
        if not download:
            return None
        idx = np.empty((self.Q, self.R), dtype=np.uint32)
        score = np.empty((self.Q, self.R), dtype=np.float32)
        check(self._lib.hg_get_topr_real(self._h, _ptr(idx), _ptr(score)))
        return idx, score

    # -- quantised databases: real-valued queries against product-quantisation codes ------
    def set_database_pq(self, codes, codebooks, labels):
        """uint8 [N, M] codes + float32 [M, K, dsub] codebooks + int64 [N, C] labels (hg_set_database_pq): the context then holds the
        sign codes of the decoded table, its labels and the PQ tables.  -> (decoded entries outside {-1,0,+1}, label entries outside {0,1})"""
        from . import pq
        codes, codebooks = pq.check_tables(codes, codebooks, values=False)      # (the library checks the values: HG_ERR_ARG names the offender)
        lab = _labels_i64(labels)
        if lab.ndim != 2 or lab.shape[0] != codes.shape[0]:
            raise ValueError("labels must be [N, C] with the codes' N")
        N, M = codes.shape
        _, K, dsub = codebooks.shape
        bc, bl = _i64(), _i64()
        check(self._lib.hg_set_database_pq(self._h, _ptr(codes), _ptr(codebooks), _ptr(lab), N, M, K, dsub, lab.shape[1], 0, N,
                                           C.byref(bc), C.byref(bl)))
        self.N, self.b, self.C, self.n_total = N, M * dsub, lab.shape[1], N
        return bc.value, bl.value

    def pq_encode(self, features, codebooks, want_err=False):
        """The exact PQ encoder on the GPU (hg_pq_encode / hg_pq_encode_dev; the contract: include/hashgan_amd.h): features a host
        array [N, M * dsub] (converted to float32) or a devarray.DeviceArray (float32 / float16 / bfloat16, any strides), codebooks
        float32 [M, K, dsub].  Needs no database and leaves the context as it was.
        -> (codes uint8 [N, M], err float64 [N] or None, rows with a non-finite feature -- their codes are 0 in that subspace)"""
        from . import pq
        cb = pq.check_codebooks(codebooks)
        M, K, dsub = cb.shape
        bad = _i64()
        if hasattr(features, "ptr"):
            f = _dev_struct(features)
            N = max(int(f.rows), 0)
            codes = np.empty((N, M), dtype=np.uint8)
            err = np.empty(N, dtype=np.float64) if want_err else None
            check(self._lib.hg_pq_encode_dev(self._h, C.byref(f), _ptr(cb), M, K, dsub, _ptr(codes), _ptr(err), C.byref(bad)))
        else:
            x = _carray(features, np.float32)
            if x.ndim != 2 or x.shape[1] != M * dsub:
                raise ValueError("features must be [N, M * dsub] = [N, %d] (have shape %r)" % (M * dsub, x.shape))
            N = x.shape[0]
            codes = np.empty((N, M), dtype=np.uint8)
            err = np.empty(N, dtype=np.float64) if want_err else None
            check(self._lib.hg_pq_encode(self._h, _ptr(x), N, _ptr(cb), M, K, dsub, _ptr(codes), _ptr(err), C.byref(bad)))
        return codes, err, bad.value

    def set_database_pq_f32(self, features, codebooks, labels):
        """float32 [N, M * dsub] features + float32 [M, K, dsub] codebooks + int64 [N, C] labels (hg_set_database_pq_f32): encoded on
        the GPU, then loaded as set_database_pq loads the codes.  ValueError, nothing loaded, when rows have a non-finite feature.
        -> (decoded entries outside {-1,0,+1}, label entries outside {0,1})"""
        from . import pq
        cb = pq.check_codebooks(codebooks)
        M, K, dsub = cb.shape
        x = _carray(features, np.float32)
        if x.ndim != 2 or x.shape[1] != M * dsub:
            raise ValueError("features must be [N, M * dsub] = [N, %d] (have shape %r)" % (M * dsub, x.shape))
        lab = _labels_i64(labels)
        if lab.ndim != 2 or lab.shape[0] != x.shape[0]:
            raise ValueError("labels must be [N, C] with the features' N")
        N = x.shape[0]
        bc, bl, br = _i64(), _i64(), _i64()
        rc = self._lib.hg_set_database_pq_f32(self._h, _ptr(x), _ptr(cb), _ptr(lab), N, M, K, dsub, lab.shape[1], 0, N,
                                              C.byref(bc), C.byref(bl), C.byref(br))
        if rc == HG_ERR_ARG and br.value:
            raise ValueError("%d feature rows are not finite: %s" % (br.value, self._lib.hg_last_error().decode("utf-8", "replace")))
        check(rc)
        self.N, self.b, self.C, self.n_total = N, M * dsub, lab.shape[1], N
        return bc.value, bl.value

    def map_pq(self, R):
        """(ap, rel) of hg_map_pq: needs set_database_pq and the queries loaded under set_option("keep_query_floats", 1)."""
        ap = np.empty(self.Q, dtype=np.float64)
        rel = np.empty(self.Q, dtype=np.int64)
        check(self._lib.hg_map_pq(self._h, int(R), _ptr(ap), _ptr(rel)))
        self.R = int(R)
        return ap, rel

    def topr_pq(self, R, download=True):
        """-> (idx, score) of hg_topr_pq through hg_get_topr_real; download=False: the lists stay on the device (graded(), votes(), export())."""
        check(self._lib.hg_topr_pq(self._h, int(R)))
        self.R = int(R)
        if not download:
            return None
        idx = np.empty((self.Q, self.R), dtype=np.uint32)
        score = np.empty((self.Q, self.R), dtype=np.float32)
        check(self._lib.hg_get_topr_real(self._h, _ptr(idx), _ptr(score)))
        return idx, score

    # -- Hamming ranking, ties re-ranked by the float inner product ---------------
    def topr_rerank(self, R, download=True):
        """Rank by (Hamming distance, inner product descending, index) -> (idx, dist, scores); download=False: the lists stay on the device."""
        check(self._lib.hg_topr_rerank(self._h, int(R)))
        self.R = int(R)
        if not download:
            return None
        idx, dist = self.get_topr()
        return idx, dist, self.get_rerank_scores()

    def map_rerank(self, R):
        ap = np.empty(self.Q, dtype=np.float64)
        rel = np.empty(self.Q, dtype=np.int64)
        check(self._lib.hg_map_rerank(self._h, int(R), _ptr(ap), _ptr(rel)))
        self.R = int(R)
        return ap, rel

    def get_rerank_scores(self):
        s = np.empty((self.Q or 0, self.R or 0), dtype=np.float32)      # (before any ranking the call is refused: nothing is written)
        check(self._lib.hg_get_rerank_scores(self._h, _ptr(s)))
        return s

    # -- results ----------------------------------------------------------------
    def get_topr(self):
        idx = np.empty((self.Q, self.R), dtype=np.uint32)
        dist = np.empty((self.Q, self.R), dtype=np.uint8)
        check(self._lib.hg_get_topr(self._h, _ptr(idx), _ptr(dist)))
        return idx, dist

    def get_match(self):
        m = np.empty((self.Q, self.R), dtype=np.uint8)
        check(self._lib.hg_get_match(self._h, _ptr(m)))
        return m

    def get_ap(self):
        ap = np.empty(self.Q, dtype=np.float64)
        rel = np.empty(self.Q, dtype=np.int64)
        check(self._lib.hg_get_ap(self._h, _ptr(ap), _ptr(rel)))
        return ap, rel

    def get_hist(self):
        h = np.empty((self.b + 1, self.Q), dtype=np.uint32)
        check(self._lib.hg_get_hist(self._h, _ptr(h)))
        return h

    def get_rel_hist(self):
        """-> (all, rel), uint32 [b+1, Q] each, of this shard (after rel_hist())."""
        shape = ((self.b or 0) + 1, self.Q or 0)          # (nothing loaded yet: the library says so)
        a = np.empty(shape, dtype=np.uint32)
        r = np.empty(shape, dtype=np.uint32)
        check(self._lib.hg_get_rel_hist(self._h, _ptr(a), _ptr(r)))
        return a, r

    def get_graded(self):
        """-> (gsum int64, hits int64, dcg float64, wsum float64), [Q, nk] each (after graded())."""
        shape = (self.Q or 0, getattr(self, "_graded_nk", 0))
        gsum, hits = np.empty(shape, dtype=np.int64), np.empty(shape, dtype=np.int64)
        dcg, wsum = np.empty(shape, dtype=np.float64), np.empty(shape, dtype=np.float64)
        check(self._lib.hg_get_graded(self._h, _ptr(gsum), _ptr(hits), _ptr(dcg), _ptr(wsum)))
        return gsum, hits, dcg, wsum

    def get_tie_ap(self):
        """-> dict(ap, p_hit, ap_min, ap_max, rel_exp float64, rel_lo, rel_hi int64), [Q, nR] each (after tie_ap())."""
        shape = (self.Q or 0, getattr(self, "_tie_nR", 0))
        f = [np.empty(shape, dtype=np.float64) for _ in range(5)]
        i = [np.empty(shape, dtype=np.int64) for _ in range(2)]
        check(self._lib.hg_get_tie_ap(self._h, *[_ptr(x) for x in f + i]))
        return dict(zip(("ap", "p_hit", "ap_min", "ap_max", "rel_exp", "rel_lo", "rel_hi"), f + i))

    def get_ap_at(self):
        """-> (ap float64 [Q, nR] with nan where the top R hold no hit, rel int64 [Q, nR]) (after ap_at())."""
        shape = (self.Q or 0, getattr(self, "_ap_at_nR", 0))
        ap = np.empty(shape, dtype=np.float64)
        rel = np.empty(shape, dtype=np.int64)
        check(self._lib.hg_get_ap_at(self._h, _ptr(ap), _ptr(rel)))
        return ap, rel

    def get_vote_pred(self):
        """-> (pred int32 [Q, nk]: the smallest class with the most votes among the top k, -1 where no retrieved row has a label;
        top int64 [Q, nk]: that class's votes) (after votes())."""
        shape = (self.Q or 0, getattr(self, "_votes_nk", 0))
        pred = np.empty(shape, dtype=np.int32)
        top = np.empty(shape, dtype=np.int64)
        check(self._lib.hg_get_vote_pred(self._h, _ptr(pred), _ptr(top)))
        return pred, top

    def get_vote_confusion(self):
        """-> int64 [nk, C, C]: conf[j, a, b] = rows of class b among the top ks[j] of the queries that carry class a (after votes())."""
        conf = np.empty((getattr(self, "_votes_nk", 0), self.C or 0, self.C or 0), dtype=np.int64)
        check(self._lib.hg_get_vote_confusion(self._h, _ptr(conf)))
        return conf

    def get_votes(self):
        """-> uint32 [Q, nk, C]: the rows of class c among the top ks[j] of query q (after votes())."""
        v = np.empty((self.Q or 0, getattr(self, "_votes_nk", 0), self.C or 0), dtype=np.uint32)
        check(self._lib.hg_get_votes(self._h, _ptr(v)))
        return v

    def get_grades(self):
        """-> uint8 [Q, R]: the grade of every rank (after graded(..., keep_grades=True))."""
        g = np.empty((self.Q or 0, self.R or 0), dtype=np.uint8)
        check(self._lib.hg_get_grades(self._h, _ptr(g)))
        return g

    def get_grade_hist(self):
        """-> uint32 [C+1, Q] of this shard (after grade_hist())."""
        h = np.empty(((self.C or 0) + 1, self.Q or 0), dtype=np.uint32)
        check(self._lib.hg_get_grade_hist(self._h, _ptr(h)))
        return h

    def get_joint_hist(self):
        """-> uint32 [b+1, G, Q] of this shard, G = stat "joint_hist_grades" (after joint_hist())."""
        h = np.empty(((self.b or 0) + 1, self.get_stat("joint_hist_grades"), self.Q or 0), dtype=np.uint32)
        check(self._lib.hg_get_joint_hist(self._h, _ptr(h)))
        return h

    # -- a shard's histogram tables: pack, (all-gather,) merge ------------------------
    def pack_side_table(self, which, Gc=0):
        """This shard's current table `which` ("rel", "grade", "joint" or an HG_SIDE_* value) as one block in the exchange layout
        (hg_pack_side_table; Gc: the grade count the ranks agreed on, joint only) -> (device address, bytes)."""
        p, n = _p(), _i64()
        check(self._lib.hg_pack_side_table(self._h, SIDE_TABLES.get(which, which), int(Gc), C.byref(p), C.byref(n)))
        return p.value, n.value

    def merge_side_table(self, which, dev_tabs_all, Gsh, Gc=0):
        """The Gsh gathered blocks summed into the whole database's table, column totals checked against n_total (hg_merge_side_table).
        Results: get_merged_rel_hist() / get_merged_grade_hist() / get_merged_joint_hist(); tie_ap() on a shard reads the rel one."""
        check(self._lib.hg_merge_side_table(self._h, SIDE_TABLES.get(which, which), _p(dev_tabs_all) if dev_tabs_all else None, int(Gsh), int(Gc)))

    def get_merged_rel_hist(self):
        """-> (all, rel), uint32 [b+1, Q] each, of the whole database (after merge_side_table("rel", ...))."""
        shape = ((self.b or 0) + 1, self.Q or 0)
        a = np.empty(shape, dtype=np.uint32)
        r = np.empty(shape, dtype=np.uint32)
        check(self._lib.hg_get_merged_rel_hist(self._h, _ptr(a), _ptr(r)))
        return a, r

    def get_merged_grade_hist(self):
        """-> uint32 [C+1, Q] of the whole database (after merge_side_table("grade", ...))."""
        h = np.empty(((self.C or 0) + 1, self.Q or 0), dtype=np.uint32)
        check(self._lib.hg_get_merged_grade_hist(self._h, _ptr(h)))
        return h

    def get_merged_joint_hist(self):
        """-> uint32 [b+1, Gc, Q] of the whole database, Gc = stat "merged_joint_grades" (after merge_side_table("joint", ...))."""
        h = np.empty(((self.b or 0) + 1, self.get_stat("merged_joint_grades"), self.Q or 0), dtype=np.uint32)
        check(self._lib.hg_get_merged_joint_hist(self._h, _ptr(h)))
        return h

    # -- a shard's part of the ranked lists: pack, (all-gather,) merge -------------------
    def pack_list_table(self, which, ks=None):
        """This shard's part of the whole database's ranked lists (a staged select with lists) as one block in the exchange layout
        (hg_pack_list_table): which = "grades" -- uint8 [Q][Rp] + uint32 own[Qpad], ks ignored -- or "votes" -- uint32 [nk][C+1][Qpad]
        at the cut-offs ks -- or an HG_LIST_* value -> (device address, bytes)."""
        p, n = _p(), _i64()
        ks = None if ks is None else _carray(ks, np.int64).ravel()
        check(self._lib.hg_pack_list_table(self._h, LIST_TABLES.get(which, which), None if ks is None else _ptr(ks), 0 if ks is None else len(ks),
                                           C.byref(p), C.byref(n)))
        return p.value, n.value

    def merge_list_table(self, which, dev_blocks_all, Gsh, ks=None):
        """The Gsh gathered blocks merged into the grade plane / the vote counts of the whole database's lists, owned slots checked
        against R and the cut-offs (hg_merge_list_table).  graded() / votes() on a shard then run from the merged table."""
        ks = None if ks is None else _carray(ks, np.int64).ravel()
        check(self._lib.hg_merge_list_table(self._h, LIST_TABLES.get(which, which), _p(dev_blocks_all) if dev_blocks_all else None, int(Gsh),
                                            None if ks is None else _ptr(ks), 0 if ks is None else len(ks)))

    # -- collectives (RCCL) -------------------------------------------------------
    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        check(self._lib.hg_comm_init(self._h, buf, int(rank), int(world)))

    def comm_destroy(self):
        check(self._lib.hg_comm_destroy(self._h))

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        check(self._lib.hg_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def allgather(self, slot, dev_ptr, nbytes):
        """-> device address of [world][nbytes], owned by the context (slot 0..3)."""
        out = _p()
        check(self._lib.hg_allgather(self._h, int(slot), _p(dev_ptr), int(nbytes), C.byref(out)))
        return out.value

    def alltoall(self, slot, dev_ptr, nbytes_per_peer):
        """dev_ptr = [world][nbytes_per_peer], block r to rank r -> device address of [world][nbytes_per_peer] received."""
        out = _p()
        check(self._lib.hg_alltoall(self._h, int(slot), _p(dev_ptr), int(nbytes_per_peer), C.byref(out)))
        return out.value

    def shard_step(self, R, replica_world=0):
        """One rank's whole step of the database-sharded bet in one call (hg_shard_step) -> (ap [Q] float64, rel [Q] int64, lost):
        lost False / True, or None when nothing was enqueued (the bet is not eligible: use the staged sequences)."""
        ap = np.empty(self.Q, dtype=np.float64)
        rel = np.empty(self.Q, dtype=np.int64)
        lost = C.c_int()
        check(self._lib.hg_shard_step(self._h, int(R), int(replica_world), _ptr(ap), _ptr(rel), C.byref(lost)))
        self.R = int(R)
        return ap, rel, (None if lost.value < 0 else bool(lost.value))

    def allgather_topr(self):
        check(self._lib.hg_allgather_topr(self._h))

    def allreduce_max(self, x):
        v = C.c_double(float(x))
        check(self._lib.hg_allreduce_max_f64(self._h, C.byref(v)))
        return v.value

    def barrier(self):
        check(self._lib.hg_barrier(self._h))

    def scratch(self, slot, nbytes):
        out = _p()
        check(self._lib.hg_scratch(self._h, int(slot), int(nbytes), C.byref(out)))
        return out.value

    def memcpy_dtod(self, dst, src, nbytes):
        check(self._lib.hg_memcpy_dtod(self._h, _p(dst), _p(src), int(nbytes)))

    def memcpy_dtoh(self, host_array, src, nbytes):
        check(self._lib.hg_memcpy_dtoh(self._h, _ptr(host_array), _p(src), int(nbytes)))

    def memcpy_htod(self, dst, host_array, nbytes):
        check(self._lib.hg_memcpy_htod(self._h, _p(dst), _ptr(host_array), int(nbytes)))

    def synchronize(self):
        check(self._lib.hg_synchronize(self._h))

    # -- tuning / timing ----------------------------------------------------------
    def set_stream(self, stream_handle):
        """Run on the caller's HIP stream (an int handle: a hipStream_t); None = back to a private one."""
        check(self._lib.hg_set_stream(self._h, _p(stream_handle) if stream_handle else None))
        self.options_touched.add("stream")

    def set_option(self, key, value):
        check(self._lib.hg_set_option(self._h, key.encode(), int(value)))
        self.options_touched.add(key)
        self.option_values[key] = int(value)

    def preload(self):
        """One-time costs of every path now instead of on first use (hg_preload)."""
        check(self._lib.hg_preload(self._h))

    def trim(self):
        """Free the work buffers (they only grow); the loaded tables stay."""
        check(self._lib.hg_trim(self._h))

    def get_stat(self, key):
        v = _i64()
        check(self._lib.hg_get_stat(self._h, key.encode(), C.byref(v)))
        return v.value

    def census(self, queries):
        """(entries outside {-1,0,+1}, zeros, minus ones, floats resident on the device) of the float table hg_set_*_f32 was handed."""
        out = (_i64 * 4)()
        check(self._lib.hg_get_census(self._h, 1 if queries else 0, out))
        return out[0], out[1], out[2], bool(out[3])

    def timing_enable(self, on=True):
        """on: False/0 off, True/2 every kernel, 1 only the select pass over the pairs (k_select, k_select_mx*) and the step's span."""
        level = 2 if on is True else (0 if on is False else int(on))
        check(self._lib.hg_timing_enable(self._h, level))

    def timing_reset(self):
        check(self._lib.hg_timing_reset(self._h))

    def timing_read(self):
        cap = 64
        names = (C.c_char_p * cap)()
        ms = (C.c_double * cap)()
        cnt = (_i64 * cap)()
        n = C.c_int()
        check(self._lib.hg_timing_read(self._h, cap, names, ms, cnt, C.byref(n)))
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n.value)}


def host_phase_timers(ctx):
    """Process-wide host-side cost of what a context does outside its kernels (hg_ctx.hpp, HostPhase): {phase: (total ms, calls,
    longest call ms)} for init, devmalloc, devfree, hostmalloc, hostfree, destroy, stream, event, sync (waiting for the GPU), pack (the host
    packing pass) and thread (starting the float table's staging thread)."""
    out = {}
    for ph in ("init", "devmalloc", "devfree", "hostmalloc", "hostfree", "destroy", "stream", "event", "sync", "pack", "thread"):
        out[ph] = (ctx.get_stat("host_us_" + ph) / 1e3, ctx.get_stat("host_n_" + ph), ctx.get_stat("host_max_us_" + ph) / 1e3)
    return out


def release_cache():
    """Return the process-wide cache of device / pinned blocks and streams to the HIP runtime (hg_release_cache)."""
    check(load().hg_release_cache())


def comm_unique_id():
    """128 opaque bytes (ncclUniqueId) for rank 0 to hand to the other ranks; loads RCCL."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    check(load().hg_comm_unique_id(buf))
    return bytes(buf)


def device_count():
    n = C.c_int()
    check(load().hg_device_count(C.byref(n)))
    return n.value


def pack_sign_f32(x):
    """float32 [n, b] -> uint64 [n, ceil(b/64)], bit = (x > 0) (hg_pack_sign_f32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, b = x.shape
    out = np.empty((n, (b + 63) // 64), dtype=np.uint64)
    check(load().hg_pack_sign_f32(_ptr(x), n, b, _ptr(out)))
    return out
