// Stand-alone check of the destination side of hashgan_amd/csrc/hg_dev_desc.hpp -- the host arithmetic behind hg_export -- meant to be
// built with -fsanitize=address,undefined on a machine without a GPU (tests/test_devout_host.py does): the condition under which no
// two elements of a destination share an address, the items' dtype and shape table, extents with the float64 item size, the
// intersection of byte ranges.  Prints "dev out check ok" and exits 0, or says which expectation failed.
#include "hg_dev_desc.hpp"

#include <climits>
#include <cstdlib>
#include <cstring>

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static hg_dev_array arr(const void* p, int64_t rows, int64_t cols, int64_t rs, int64_t cs, int dtype) {
    hg_dev_array a;
    memset(&a, 0, sizeof a);
    a.ptr = p; a.rows = rows; a.cols = cols; a.row_stride = rs; a.col_stride = cs; a.dtype = dtype;
    return a;
}
static hg_export_item item(int what, const hg_dev_array& a) {
    hg_export_item it;
    memset(&it, 0, sizeof it);
    it.what = what; it.dst = a;
    return it;
}

// Brute force over a small array: does any address occur twice?
static bool aliases(int64_t rows, int64_t cols, int64_t rs, int64_t cs) {
    static bool seen[4096];
    memset(seen, 0, sizeof seen);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) {
            const int64_t at = r * rs + c * cs;
            if (at >= 4096) abort();
            if (seen[at]) return true;
            seen[at] = true;
        }
    return false;
}

int main() {
    using namespace hg_dev;
    alignas(16) static char mem[256];
    int64_t e = -1;
    char msg[256];

    // item sizes: float64 is there, the loaders' dtype classes do not know it
    EXPECT(itemsize(HG_F64) == 8 && !feature_dtype(HG_F64) && !label_dtype(HG_F64) && strcmp(dtype_name(HG_F64), "float64") == 0);
    EXPECT(extent_bytes(arr(mem, 5, 1, 1, 1, HG_F64), &e) && e == 40);
    EXPECT(extent_bytes(arr(mem, 5, 7, 9, 1, HG_I64), &e) && e == (4 * 9 + 7) * 8);
    EXPECT(!extent_bytes(arr(mem, 2, 1, INT64_MAX / 4, 1, HG_F64), &e));                   // times the item size
    {
        hg_dev_array f = arr(mem, 4, 4, 4, 1, HG_F64), l = arr(mem, 4, 4, 4, 1, HG_I64);
        int64_t fb = 0, lb = 0;
        EXPECT(check_pair(&f, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr && strstr(msg, "float64"));
        f = arr(mem, 4, 4, 4, 1, HG_F32); l = arr(mem, 4, 4, 4, 1, HG_F64);
        EXPECT(check_pair(&f, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr && strstr(msg, "float64"));
    }

    // disjoint writes: contiguous, row pitch > cols, column stride 2, transposed, one row, one column
    EXPECT(writes_disjoint(arr(mem, 5, 7, 7, 1, HG_I64)));
    EXPECT(writes_disjoint(arr(mem, 5, 7, 10, 1, HG_I64)));
    EXPECT(writes_disjoint(arr(mem, 5, 7, 14, 2, HG_I64)) && writes_disjoint(arr(mem, 5, 7, 13, 2, HG_I64)));
    EXPECT(writes_disjoint(arr(mem, 5, 7, 1, 5, HG_I64)) && writes_disjoint(arr(mem, 5, 7, 2, 9, HG_I64)));
    EXPECT(writes_disjoint(arr(mem, 1, 7, 1, 1, HG_I64)) && writes_disjoint(arr(mem, 1, 7, INT64_MAX, 3, HG_I64)));
    EXPECT(writes_disjoint(arr(mem, 5, 1, 1, 1, HG_I64)) && writes_disjoint(arr(mem, 5, 1, 2, INT64_MAX, HG_I64)));
    EXPECT(writes_disjoint(arr(mem, 1, 1, 1, 1, HG_U8)));
    // elements that alias
    EXPECT(!writes_disjoint(arr(mem, 2, 2, 1, 1, HG_I64)));
    EXPECT(!writes_disjoint(arr(mem, 3, 3, 2, 1, HG_I64)));
    EXPECT(!writes_disjoint(arr(mem, 5, 7, 6, 1, HG_I64)) && !writes_disjoint(arr(mem, 5, 7, 1, 4, HG_I64)) && !writes_disjoint(arr(mem, 3, 3, 2, 2, HG_I64)));
    // malformed
    EXPECT(!writes_disjoint(arr(mem, 0, 2, 2, 1, HG_I64)) && !writes_disjoint(arr(mem, 2, 2, 0, 1, HG_I64)) && !writes_disjoint(arr(mem, 2, 2, 2, -1, HG_I64)));
    // strides next to 2^63: judged, not overflowed
    EXPECT(writes_disjoint(arr(mem, 2, 2, INT64_MAX, 1, HG_U8)));                          // row_stride > 1 * 1 (its extent does not fit: see below)
    EXPECT(!writes_disjoint(arr(mem, 3, 3, INT64_MAX, INT64_MAX, HG_U8)));                 // both products overflow
    EXPECT(!writes_disjoint(arr(mem, 3, 3, INT64_MAX / 2 + 1, INT64_MAX / 2 + 1, HG_U8)));
    EXPECT(!writes_disjoint(arr(mem, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX, HG_U8)));
    EXPECT(writes_disjoint(arr(mem, 3, 3, INT64_MAX, INT64_MAX / 2, HG_U8)));              // 2 * (2^62 - 1) < 2^63 - 1
    // the rule is exact on a sweep of small arrays where it accepts, and never accepts an aliasing one
    for (int64_t rows = 1; rows <= 4; ++rows)
        for (int64_t cols = 1; cols <= 4; ++cols)
            for (int64_t rs = 1; rs <= 9; ++rs)
                for (int64_t cs = 1; cs <= 9; ++cs)
                    if (writes_disjoint(arr(mem, rows, cols, rs, cs, HG_U8))) EXPECT(!aliases(rows, cols, rs, cs));

    // the items' dtype table
    const int dtypes[] = {HG_F32, HG_F16, HG_BF16, HG_I64, HG_I32, HG_U8, HG_F64, 7, -1};
    for (int d : dtypes) {
        EXPECT(out_dtype_ok(HG_OUT_IDX, d) == (d == HG_I64 || d == HG_I32));
        EXPECT(out_dtype_ok(HG_OUT_HITS, d) == (d == HG_I64 || d == HG_I32));
        EXPECT(out_dtype_ok(HG_OUT_DIST, d) == (d == HG_U8 || d == HG_I32));
        EXPECT(out_dtype_ok(HG_OUT_GRADES, d) == (d == HG_U8 || d == HG_I32));
        EXPECT(out_dtype_ok(HG_OUT_SCORE, d) == (d == HG_F32));
        EXPECT(out_dtype_ok(HG_OUT_MATCH, d) == (d == HG_U8));
        EXPECT(out_dtype_ok(HG_OUT_AP, d) == (d == HG_F64 || d == HG_F32));
        EXPECT(!out_dtype_ok(7, d) && !out_dtype_ok(-1, d));
    }

    // the item checks: Q = 5 queries, lists of R = 130, a database of 400 rows
    const int64_t Q = 5, R = 130, N = 400;
    int64_t nb = 0;
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, R, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) == nullptr && nb == Q * R * 8);
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, 17, R + 3, 1, HG_I32)), Q, R, N, &nb, msg, sizeof msg) == nullptr && nb == (4 * (R + 3) + 17) * 4);
    EXPECT(check_out_item(item(HG_OUT_MATCH, arr(mem, Q, R, 1, Q, HG_U8)), Q, R, N, &nb, msg, sizeof msg) == nullptr && nb == Q * R);
    EXPECT(check_out_item(item(HG_OUT_AP, arr(mem, Q, 1, 1, 1, HG_F64)), Q, 1, N, &nb, msg, sizeof msg) == nullptr && nb == Q * 8);
    EXPECT(check_out_item(item(HG_OUT_AP, arr(mem, Q, 1, 3, 1, HG_F32)), Q, 1, N, &nb, msg, sizeof msg) == nullptr && nb == (4 * 3 + 1) * 4);
    EXPECT(check_out_item(item(HG_OUT_HITS, arr(mem, Q, 1, 1, 1, HG_I64)), Q, 1, N, &nb, msg, sizeof msg) == nullptr);
    EXPECT(check_out_item(item(HG_OUT_GRADES, arr(mem, Q, R, R, 1, HG_U8)), Q, R, N, &nb, msg, sizeof msg) == nullptr && nb == Q * R);
    // refused
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, R, 1, HG_F32)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "float32"));
    EXPECT(check_out_item(item(HG_OUT_AP, arr(mem, Q, 1, 1, 1, HG_I64)), Q, 1, N, &nb, msg, sizeof msg) != nullptr);
    EXPECT(check_out_item(item(HG_OUT_SCORE, arr(mem, Q, R, R, 1, HG_F64)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "float64"));
    EXPECT(check_out_item(item(7, arr(mem, Q, R, R, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr);
    EXPECT(check_out_item(item(-1, arr(mem, Q, R, R, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr);
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(nullptr, Q, R, R, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "null"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q + 1, R, R, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "rows"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R + 1, R + 1, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "columns"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, 0, R, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr);
    EXPECT(check_out_item(item(HG_OUT_AP, arr(mem, Q, 2, 2, 1, HG_F64)), Q, 1, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "columns"));
    EXPECT(check_out_item(item(HG_OUT_HITS, arr(mem, Q, 2, 2, 1, HG_I64)), Q, 1, N, &nb, msg, sizeof msg) != nullptr);
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, 0, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "strides"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, R, -1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "strides"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, 2, 2, 1, 1, HG_I64)), 2, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "share an address"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, 3, 3, 2, 1, HG_I64)), 3, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "share an address"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, INT64_MAX, 1, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "63 bits"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, INT64_MAX / 2, INT64_MAX / 2, HG_I64)), Q, R, N, &nb, msg, sizeof msg) != nullptr);
    EXPECT(check_out_item(item(HG_OUT_MATCH, arr(mem, Q, R, INT64_MAX / 4, 1, HG_U8)), Q, R, N, &nb, msg, sizeof msg) != nullptr && strstr(msg, "63 bits"));
    // IDX as int32 against the database's size
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, R, 1, HG_I32)), Q, R, (int64_t)INT32_MAX, &nb, msg, sizeof msg) == nullptr);
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, R, 1, HG_I32)), Q, R, (int64_t)INT32_MAX + 1, &nb, msg, sizeof msg) != nullptr && strstr(msg, "2^31"));
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, Q, R, R, 1, HG_I64)), Q, R, (int64_t)INT32_MAX + 1, &nb, msg, sizeof msg) == nullptr);
    EXPECT(check_out_item(item(HG_OUT_HITS, arr(mem, Q, 1, 1, 1, HG_I32)), Q, 1, (int64_t)INT32_MAX + 1, &nb, msg, sizeof msg) == nullptr);
    char tiny[8];                                                                           // (a short message buffer is not overrun)
    EXPECT(check_out_item(item(HG_OUT_IDX, arr(mem, 2, 2, 1, 1, HG_I64)), 2, R, N, &nb, tiny, sizeof tiny) != nullptr && strlen(tiny) < sizeof tiny);

    // the 16-byte store path asks what the load path asks
    EXPECT(vector_stores_ok(arr(mem, 5, 37, 40, 1, HG_I64)) && !vector_stores_ok(arr(mem + 8, 5, 37, 40, 1, HG_I64)) && !vector_stores_ok(arr(mem, 5, 37, 37, 1, HG_I32)));
    EXPECT(vector_stores_ok(arr(mem, 5, 37, 48, 1, HG_U8)) && !vector_stores_ok(arr(mem, 5, 37, 40, 1, HG_U8)) && !vector_stores_ok(arr(mem, 5, 37, 74, 2, HG_I64)));

    // byte ranges
    EXPECT(ranges_intersect(mem, 16, mem + 15, 1) && !ranges_intersect(mem, 16, mem + 16, 1) && ranges_intersect(mem + 15, 1, mem, 16));
    EXPECT(!ranges_intersect(mem + 16, 1, mem, 16) && ranges_intersect(mem, 64, mem + 8, 8) && ranges_intersect(mem + 8, 8, mem, 64));
    EXPECT(ranges_intersect(mem, 1, mem, 1) && !ranges_intersect(mem, 0, mem, 16) && !ranges_intersect(mem, 16, mem + 4, 0));
    EXPECT(ranges_intersect((const void*)16, INT64_MAX, (const void*)(UINTPTR_MAX - 1), 1) == false);      // 16 + 2^63 - 1 < 2^64 - 2
    EXPECT(ranges_intersect((const void*)(UINTPTR_MAX - 7), 8, (const void*)(UINTPTR_MAX - 3), 4));        // ranges that end at the top
    EXPECT(!ranges_intersect((const void*)(UINTPTR_MAX - 7), 4, (const void*)(UINTPTR_MAX - 3), 4));

    if (failures) { printf("%d expectation(s) failed\n", failures); return 1; }
    printf("dev out check ok\n");
    return 0;
}
