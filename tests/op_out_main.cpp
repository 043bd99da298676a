/* Stand-alone exerciser of arroyo_amd/csrc/op_out.h, built by
 * tests/test_op_out_host.py with -fsanitize=address,undefined and run as a
 * child process.  Exits 0 when every check holds. */
#include <cstdio>

#include "../arroyo_amd/csrc/op_out.h"

/* a malloc the allocator cannot serve returns NULL instead of aborting, so
 * the failure path of out_alloc is reachable under ASan */
extern "C" const char *__asan_default_options() {
    return "allocator_may_return_null=1";
}

static int failures;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__,  \
                    #cond);                                                   \
            failures++;                                                       \
        }                                                                     \
    } while (0)

static bool all_zero(const AmdOutBatch &b) {
    const unsigned char *p = (const unsigned char *)&b;
    for (size_t i = 0; i < sizeof b; i++)
        if (p[i]) return false;
    return true;
}

int main() {
    const int64_t rows[] = {0, 1};
    const int ncols[] = {1, 16};
    for (int64_t n : rows)
        for (int nc : ncols) {
            AmdOutBatch b;
            memset(&b, 0xAB, sizeof b); /* out_alloc must not trust it */
            CHECK(out_alloc(&b, n, nc) == 0);
            CHECK(b.n_rows == n && b.n_cols == nc && !b.on_device);
            CHECK(b.cols && b.is_f64 && !b.validity);
            for (int c = 0; c < nc; c++) {
                CHECK(b.cols[c] != nullptr);
                CHECK(b.is_f64[c] == 0);
                /* the whole column (one element at least) is writable */
                memset(b.cols[c], 0x5A, (size_t)(n ? n : 1) * 8);
            }
            CHECK(out_alloc_validity(&b) == 0);
            CHECK(b.validity != nullptr);
            for (int c = 0; c < nc; c++) CHECK(b.validity[c] == nullptr);
            /* a bitmap on the first and the last column, the rest all-valid */
            const int with_bm[] = {0, nc - 1};
            for (int c : with_bm) {
                uint8_t *bm = out_validity_col(&b, c);
                CHECK(bm != nullptr && bm == b.validity[c]);
                for (int64_t i = 0; bm && i < (n + 7) / 8; i++)
                    CHECK(bm[i] == 0);
                if (bm && n) bm[(n - 1) >> 3] |= (uint8_t)(1u << ((n - 1) & 7));
            }
            out_free_host(&b);
            CHECK(all_zero(b));
            out_free_host(&b); /* free after zero: a no-op */
            CHECK(all_zero(b));
        }

    /* a batch without a validity table frees too */
    AmdOutBatch plain;
    CHECK(out_alloc(&plain, 1, 1) == 0);
    out_free_host(&plain);
    CHECK(all_zero(plain));
    out_free_host(nullptr);

    /* failure path: a column size no allocator can serve, and sizes whose
     * byte count does not fit size_t or is negative */
    const int64_t bad_rows[] = {INT64_MAX / 16, INT64_MAX, -1};
    for (int64_t n : bad_rows) {
        AmdOutBatch b;
        memset(&b, 0xAB, sizeof b);
        CHECK(out_alloc(&b, n, 16) != 0);
        CHECK(all_zero(b));
        out_free_host(&b);
        CHECK(all_zero(b));
    }
    if (failures) return 1;
    puts("op_out: ok");
    return 0;
}
