// Stand-alone check of hashgan_amd/csrc/hg_dev_desc.hpp -- the host arithmetic behind hg_set_database_dev / hg_set_queries_dev --
// meant to be built with -fsanitize=address,undefined on a machine without a GPU (tests/test_devarray_host.py does):
// extents at the edges (one row, one column, unit strides, sums next to 2^63), the 16-byte-load condition, the descriptor
// checks and the inside-the-allocation test.  Prints "dev array check ok" and exits 0, or says which expectation failed.
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

int main() {
    using namespace hg_dev;
    alignas(16) static char mem[64];
    int64_t e = -1;

    // item sizes and dtype classes
    EXPECT(itemsize(HG_F32) == 4 && itemsize(HG_F16) == 2 && itemsize(HG_BF16) == 2 && itemsize(HG_I64) == 8 && itemsize(HG_I32) == 4 &&
           itemsize(HG_U8) == 1 && itemsize(17) == 0 && itemsize(-1) == 0);
    EXPECT(feature_dtype(HG_F32) && feature_dtype(HG_F16) && feature_dtype(HG_BF16) && !feature_dtype(HG_I64) && !feature_dtype(HG_U8));
    EXPECT(label_dtype(HG_I64) && label_dtype(HG_I32) && label_dtype(HG_U8) && label_dtype(HG_F32) && !label_dtype(HG_F16) && !label_dtype(HG_BF16));

    // extents: contiguous, pitched, transposed, one row, one column, both strides > 1
    EXPECT(extent_bytes(arr(mem, 37, 33, 33, 1, HG_F32), &e) && e == 37 * 33 * 4);
    EXPECT(extent_bytes(arr(mem, 37, 33, 40, 1, HG_F32), &e) && e == (36 * 40 + 33) * 4);
    EXPECT(extent_bytes(arr(mem, 37, 33, 1, 37, HG_F16), &e) && e == (36 + 32 * 37 + 1) * 2);
    EXPECT(extent_bytes(arr(mem, 1, 1, 1, 1, HG_U8), &e) && e == 1);
    EXPECT(extent_bytes(arr(mem, 1, 255, INT64_MAX, 1, HG_BF16), &e) && e == 255 * 2);      // one row: its pitch is never applied
    EXPECT(extent_bytes(arr(mem, 5, 1, 1, INT64_MAX, HG_I64), &e) && e == 5 * 8);
    EXPECT(extent_bytes(arr(mem, 3, 4, 10, 2, HG_I32), &e) && e == (2 * 10 + 3 * 2 + 1) * 4);
    // malformed
    EXPECT(!extent_bytes(arr(mem, 0, 4, 4, 1, HG_F32), &e) && !extent_bytes(arr(mem, 4, 0, 4, 1, HG_F32), &e));
    EXPECT(!extent_bytes(arr(mem, 4, 4, 0, 1, HG_F32), &e) && !extent_bytes(arr(mem, 4, 4, 4, 0, HG_F32), &e));
    EXPECT(!extent_bytes(arr(mem, 4, 4, -4, 1, HG_F32), &e) && !extent_bytes(arr(mem, 4, 4, 4, 1, 99), &e));
    // next to 2^63: the largest that fits, and every step of the sum overflowing
    EXPECT(extent_bytes(arr(mem, 2, 1, INT64_MAX - 1, 1, HG_U8), &e) && e == INT64_MAX);
    EXPECT(!extent_bytes(arr(mem, 2, 1, INT64_MAX, 1, HG_U8), &e));                         // the + 1
    EXPECT(!extent_bytes(arr(mem, 3, 1, INT64_MAX / 2 + 1, 1, HG_U8), &e));                 // (rows - 1) * row_stride
    EXPECT(!extent_bytes(arr(mem, 1, 3, 1, INT64_MAX / 2 + 1, HG_U8), &e));                 // (cols - 1) * col_stride
    EXPECT(!extent_bytes(arr(mem, 2, 2, INT64_MAX / 2 + 1, INT64_MAX / 2 + 1, HG_U8), &e)); // their sum
    EXPECT(!extent_bytes(arr(mem, 2, 1, INT64_MAX / 4, 1, HG_I64), &e));                    // times the item size
    EXPECT(extent_bytes(arr(mem, 2, 1, INT64_MAX / 8 - 1, 1, HG_I64), &e) && e == (INT64_MAX / 8) * 8);
    EXPECT(!extent_bytes(arr(mem, INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX, HG_I64), &e));

    // 16-byte loads: unit column stride, aligned base, pitch a multiple of 16 bytes (any pitch for one row)
    EXPECT(vector_loads_ok(arr(mem, 8, 64, 64, 1, HG_F32)) && vector_loads_ok(arr(mem, 8, 33, 36, 1, HG_F32)));
    EXPECT(!vector_loads_ok(arr(mem, 8, 33, 33, 1, HG_F32)) && !vector_loads_ok(arr(mem + 4, 8, 64, 64, 1, HG_F32)));
    EXPECT(!vector_loads_ok(arr(mem, 8, 64, 128, 2, HG_F32)) && !vector_loads_ok(arr(mem, 8, 8, 1, 8, HG_F32)));
    EXPECT(vector_loads_ok(arr(mem, 8, 64, 64, 1, HG_F16)) && !vector_loads_ok(arr(mem, 8, 60, 60, 1, HG_F16)) && !vector_loads_ok(arr(mem + 2, 8, 64, 64, 1, HG_BF16)));
    EXPECT(vector_loads_ok(arr(mem, 1, 33, 33, 1, HG_F32)) && vector_loads_ok(arr(mem, 1, 33, INT64_MAX, 1, HG_F32)));

    // the pair checks, in the order the entry points rely on
    char msg[256];
    int64_t fb = 0, lb = 0;
    hg_dev_array f = arr(mem, 37, 33, 33, 1, HG_F32), l = arr(mem, 37, 65, 65, 1, HG_I64);
    EXPECT(check_pair(&f, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) == nullptr && fb == 37 * 33 * 4 && lb == 37 * 65 * 8);
    EXPECT(check_pair(&f, &l, HG_MAX_BITS, 1000, 33, 65, &fb, &lb, msg, sizeof msg) == nullptr);
    EXPECT(check_pair(&f, &l, HG_MAX_BITS, 1000, 32, 65, &fb, &lb, msg, sizeof msg) != nullptr);
    EXPECT(check_pair(&f, &l, HG_MAX_BITS, 36, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr);
    EXPECT(check_pair(nullptr, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr);
    hg_dev_array g = f;
    g.dtype = HG_I64;
    EXPECT(check_pair(&g, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr && strstr(msg, "int64"));
    g = f; g.col_stride = 0;
    EXPECT(check_pair(&g, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr && strstr(msg, "stride"));
    g = f; g.row_stride = -33;
    EXPECT(check_pair(&g, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr);
    g = f; g.rows = 36;
    EXPECT(check_pair(&g, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr && strstr(msg, "rows"));
    g = f; g.cols = 256;
    EXPECT(check_pair(&g, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr);
    g = f; g.ptr = nullptr;
    EXPECT(check_pair(&g, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr);
    g = l; g.dtype = HG_BF16;
    EXPECT(check_pair(&f, &g, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr);
    g = f; g.row_stride = INT64_MAX;
    EXPECT(check_pair(&g, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, msg, sizeof msg) != nullptr && strstr(msg, "63 bits"));
    char tiny[8];                                                                           // (a short message buffer is not overrun)
    EXPECT(check_pair(&g, &l, HG_MAX_BITS, 1000, 0, 0, &fb, &lb, tiny, sizeof tiny) != nullptr && strlen(tiny) < sizeof tiny);

    // inside the allocation
    EXPECT(inside(mem, 64, mem, 64) && !inside(mem, 65, mem, 64) && inside(mem + 60, 4, mem, 64) && !inside(mem + 61, 4, mem, 64));
    EXPECT(!inside(mem, 1, mem + 1, 63) && inside(mem + 64, 0, mem, 64) && !inside(mem + 65, 0, mem, 64) && !inside(mem, -1, mem, 64));
    EXPECT(!inside(mem, INT64_MAX, mem, 64) && !inside((const void*)UINTPTR_MAX, 2, (const void*)(UINTPTR_MAX - 1), 1));

    if (failures) { printf("%d expectation(s) failed\n", failures); return 1; }
    printf("dev array check ok\n");
    return 0;
}
