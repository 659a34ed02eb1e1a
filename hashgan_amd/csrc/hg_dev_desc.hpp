// Host-side arithmetic on hg_dev_array descriptors (include/hashgan_amd.h): item sizes, dtype classes, the byte extent an array
// spans, the condition for the 16-byte load path, and the checks hg_set_database_dev / hg_set_queries_dev make before they ask the
// HIP runtime about the pointer; for hg_export's destinations the dtype and shape table of the items, the condition under which no
// two elements share an address, and the intersection of two byte ranges (tests/dev_out_check.cpp runs those the same way).  Plain C++ without a HIP include, so that tests/dev_array_check.cpp can run it under
// -fsanitize=address,undefined on a machine without a GPU (tests/test_devarray_host.py).
#pragma once
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "../../include/hashgan_amd.h"

namespace hg_dev {

inline int itemsize(int dtype) {
    switch (dtype) {
        case HG_F32: case HG_I32: return 4;
        case HG_F16: case HG_BF16: return 2;
        case HG_I64: case HG_F64: return 8;
        case HG_U8: return 1;
        default: return 0;
    }
}
inline bool feature_dtype(int d) { return d == HG_F32 || d == HG_F16 || d == HG_BF16; }
inline bool label_dtype(int d) { return d == HG_I64 || d == HG_I32 || d == HG_U8 || d == HG_F32; }
inline const char* dtype_name(int d) {
    switch (d) {
        case HG_F32: return "float32"; case HG_F16: return "float16"; case HG_BF16: return "bfloat16";
        case HG_I64: return "int64"; case HG_I32: return "int32"; case HG_U8: return "uint8"; case HG_F64: return "float64";
        default: return "unknown";
    }
}

// Bytes from a.ptr to one past the last element: ((rows-1)*row_stride + (cols-1)*col_stride + 1) * itemsize.  false when the
// descriptor is malformed (rows / cols / strides < 1, unknown dtype) or the sum does not fit an int64: a kernel's index
// arithmetic (int64 element offsets) is safe exactly when this succeeds.
inline bool extent_bytes(const hg_dev_array& a, int64_t* out) {
    const int isz = itemsize(a.dtype);
    if (!isz || a.rows < 1 || a.cols < 1 || a.row_stride < 1 || a.col_stride < 1) return false;
    int64_t r = 0, c = 0, e = 0;
    if (__builtin_mul_overflow(a.rows - 1, a.row_stride, &r)) return false;
    if (__builtin_mul_overflow(a.cols - 1, a.col_stride, &c)) return false;
    if (__builtin_add_overflow(r, c, &e)) return false;
    if (__builtin_add_overflow(e, (int64_t)1, &e)) return false;
    if (__builtin_mul_overflow(e, (int64_t)isz, &e)) return false;
    *out = e;
    return true;
}

// 16-byte loads along a row: unit column stride, base and row pitch (in bytes) multiples of 16.  (The pitch of a one-row array
// is never applied; the product is taken modulo 2^64, which keeps it modulo 16.)
inline bool vector_loads_ok(const hg_dev_array& a) {
    const uint64_t pitch = (uint64_t)a.row_stride * (uint64_t)itemsize(a.dtype);
    return a.col_stride == 1 && ((uintptr_t)a.ptr & 15) == 0 && (a.rows == 1 || (pitch & 15) == 0);
}

// Everything about a (features, labels) pair that can be judged without the runtime.  nullptr: fine; otherwise the complaint
// (in msg).  max_rows: the callers' row limit; want_b / want_C: the database's widths the queries must match (0: any).
inline const char* check_pair(const hg_dev_array* f, const hg_dev_array* l, int max_bits, int64_t max_rows, int want_b, int want_C,
                              int64_t* f_bytes, int64_t* l_bytes, char* msg, size_t cap) {
    if (!f || !l) { snprintf(msg, cap, "null descriptor"); return msg; }
    if (!f->ptr || !l->ptr) { snprintf(msg, cap, "null data pointer"); return msg; }
    if (!feature_dtype(f->dtype)) {
        snprintf(msg, cap, "feature dtype %d (%s) is not float32, float16 or bfloat16", f->dtype, dtype_name(f->dtype));
        return msg;
    }
    if (!label_dtype(l->dtype)) {
        snprintf(msg, cap, "label dtype %d (%s) is not int64, int32, uint8 or float32", l->dtype, dtype_name(l->dtype));
        return msg;
    }
    for (const hg_dev_array* a : {f, l}) {
        if (a->row_stride < 1 || a->col_stride < 1) {
            snprintf(msg, cap, "%s strides (%lld, %lld) must both be >= 1 (in elements)", a == f ? "feature" : "label",
                     (long long)a->row_stride, (long long)a->col_stride);
            return msg;
        }
    }
    if (f->rows < 1 || f->rows > max_rows) { snprintf(msg, cap, "%lld rows outside 1..%lld", (long long)f->rows, (long long)max_rows); return msg; }
    if (l->rows != f->rows) {
        snprintf(msg, cap, "features have %lld rows, labels %lld", (long long)f->rows, (long long)l->rows);
        return msg;
    }
    if (f->cols < 1 || f->cols > max_bits) { snprintf(msg, cap, "b=%lld outside 1..%d", (long long)f->cols, max_bits); return msg; }
    if (l->cols < 1 || l->cols > INT32_MAX) { snprintf(msg, cap, "C=%lld", (long long)l->cols); return msg; }
    if ((want_b && f->cols != want_b) || (want_C && l->cols != want_C)) {
        snprintf(msg, cap, "b=%lld, C=%lld do not match the database (b=%d, C=%d)", (long long)f->cols, (long long)l->cols, want_b, want_C);
        return msg;
    }
    if (!extent_bytes(*f, f_bytes) || !extent_bytes(*l, l_bytes)) {
        snprintf(msg, cap, "the array's extent in bytes does not fit 63 bits");
        return msg;
    }
    return nullptr;
}

// Does [ptr, ptr + extent) lie inside the allocation [base, base + size)?
inline bool inside(const void* ptr, int64_t extent, const void* base, size_t size) {
    const uintptr_t p = (uintptr_t)ptr, b0 = (uintptr_t)base;
    if (extent < 0 || p < b0) return false;
    const uintptr_t off = p - b0;
    return off <= size && (uint64_t)extent <= (uint64_t)(size - off);
}

// ---- destinations of hg_export ----------------------------------------------------------------------------------------------
// The 16-byte store path asks of a destination what the 16-byte load path asks of a source.
inline bool vector_stores_ok(const hg_dev_array& a) { return vector_loads_ok(a); }

// No two elements of the array share an address: one row or one column, or the rows do not reach into each other
// (row_stride > (cols-1)*col_stride), or the columns do not (col_stride > (rows-1)*row_stride) -- every slice or transpose of a
// contiguous array.  A product that overflows is larger than any stride.  (rows, cols, strides >= 1: extent_bytes has checked.)
inline bool writes_disjoint(const hg_dev_array& a) {
    if (a.rows < 1 || a.cols < 1 || a.row_stride < 1 || a.col_stride < 1) return false;
    if (a.rows == 1 || a.cols == 1) return true;
    int64_t span = 0;
    if (!__builtin_mul_overflow(a.cols - 1, a.col_stride, &span) && a.row_stride > span) return true;
    if (!__builtin_mul_overflow(a.rows - 1, a.row_stride, &span) && a.col_stride > span) return true;
    return false;
}

// Do [p, p + n) and [q, q + m) share a byte?  (n, m >= 0; ranges that end at the top of the address space included)
inline bool ranges_intersect(const void* p, int64_t n, const void* q, int64_t m) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    if (n <= 0 || m <= 0) return false;
    return a < b ? (uint64_t)n > (uint64_t)(b - a) : (uint64_t)m > (uint64_t)(a - b);
}

inline const char* out_name(int what) {
    switch (what) {
        case HG_OUT_IDX: return "IDX"; case HG_OUT_DIST: return "DIST"; case HG_OUT_SCORE: return "SCORE"; case HG_OUT_MATCH: return "MATCH";
        case HG_OUT_AP: return "AP"; case HG_OUT_HITS: return "HITS"; case HG_OUT_GRADES: return "GRADES";
        default: return "unknown";
    }
}
// the dtypes an item may be written as
inline bool out_dtype_ok(int what, int d) {
    switch (what) {
        case HG_OUT_IDX: case HG_OUT_HITS: return d == HG_I64 || d == HG_I32;
        case HG_OUT_DIST: case HG_OUT_GRADES: return d == HG_U8 || d == HG_I32;
        case HG_OUT_SCORE: return d == HG_F32;
        case HG_OUT_MATCH: return d == HG_U8;
        case HG_OUT_AP: return d == HG_F64 || d == HG_F32;
        default: return false;
    }
}
inline bool out_per_query(int what) { return what == HG_OUT_AP || what == HG_OUT_HITS; }

// Everything about one item that can be judged without the runtime.  nullptr: fine, *bytes = the destination's extent; otherwise
// the complaint (in msg).  Q, R: rows and list length of the result the item reads; n_total: the database's rows (IDX as int32).
inline const char* check_out_item(const hg_export_item& it, int64_t Q, int64_t R, int64_t n_total, int64_t* bytes, char* msg, size_t cap) {
    const hg_dev_array& a = it.dst;
    const char* nm = out_name(it.what);
    if (it.what < HG_OUT_IDX || it.what > HG_OUT_GRADES) { snprintf(msg, cap, "unknown item %d", it.what); return msg; }
    if (!a.ptr) { snprintf(msg, cap, "%s: null data pointer", nm); return msg; }
    if (!out_dtype_ok(it.what, a.dtype)) {
        snprintf(msg, cap, "%s cannot be written as dtype %d (%s)", nm, a.dtype, dtype_name(a.dtype));
        return msg;
    }
    if (a.row_stride < 1 || a.col_stride < 1) {
        snprintf(msg, cap, "%s: strides (%lld, %lld) must both be >= 1 (in elements)", nm, (long long)a.row_stride, (long long)a.col_stride);
        return msg;
    }
    if (a.rows != Q) { snprintf(msg, cap, "%s: %lld rows, the results have %lld queries", nm, (long long)a.rows, (long long)Q); return msg; }
    if (out_per_query(it.what) ? a.cols != 1 : (a.cols < 1 || a.cols > R)) {
        snprintf(msg, cap, "%s: %lld columns outside 1..%lld", nm, (long long)a.cols, (long long)(out_per_query(it.what) ? 1 : R));
        return msg;
    }
    if (it.what == HG_OUT_IDX && a.dtype == HG_I32 && n_total > (int64_t)INT32_MAX) {
        snprintf(msg, cap, "IDX as int32: the database has %lld rows (more than 2^31 - 1)", (long long)n_total);
        return msg;
    }
    if (!extent_bytes(a, bytes)) { snprintf(msg, cap, "%s: the array's extent in bytes does not fit 63 bits", nm); return msg; }
    if (!writes_disjoint(a)) {
        snprintf(msg, cap, "%s: strides (%lld, %lld) make elements of a [%lld, %lld] array share an address", nm, (long long)a.row_stride,
                 (long long)a.col_stride, (long long)a.rows, (long long)a.cols);
        return msg;
    }
    return nullptr;
}

}  // namespace hg_dev
