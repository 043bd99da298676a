/* Stand-alone driver for the map section of oracle/arroyo_oracle.c, built
 * with AddressSanitizer + UBSan by tests/test_map_oracle_host.py and run as
 * a child process.  It walks oracle_map_* through the corners where the
 * arithmetic used to be undefined behaviour (signed wrap, INT64_MIN / -1 and
 * % -1, F2I out of range), through the error return (whose output batch
 * LeakSanitizer watches) and through a rejected config.  Prints
 * "map_oracle: ok" when every check held. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/arroyo_amd_types.h"

void *oracle_map_create(const AmdMapConfig *cfg);
const char *oracle_map_last_error(void *h);
int oracle_map_process_batch(void *h, const int64_t *const *cols,
                             int32_t n_cols, int64_t n_rows, AmdOutBatch *out);
void oracle_map_destroy(void *h);
void oracle_free_out(AmdOutBatch *out);

static int failures;

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond);   \
            failures++;                                                       \
        }                                                                     \
    } while (0)

static int64_t bits(double d) { int64_t b; memcpy(&b, &d, 8); return b; }

/* r2 = op(r0, r1) over two input columns, one output */
static AmdMapConfig binary(int op) {
    AmdMapConfig c;
    memset(&c, 0, sizeof c);
    c.n_in_cols = 2;
    c.n_prog = 1;
    c.prog[0].op = op;
    c.prog[0].a = 0;
    c.prog[0].b = 1;
    c.prog[0].dst = 2;
    c.n_out = 1;
    c.out_reg[0] = 2;
    c.filter_reg = -1;
    return c;
}

/* run `op` over n (a, b) rows; returns 0 and fills got[], or 1 with the
 * handle's message copied to msg */
static int run(int op, const int64_t *a, const int64_t *b, int64_t n,
               int64_t *got, char *msg) {
    AmdMapConfig c = binary(op);
    void *h = oracle_map_create(&c);
    CHECK(h != NULL);
    if (!h) return 1;
    const int64_t *cols[2] = {a, b};
    AmdOutBatch out;
    int rc = oracle_map_process_batch(h, cols, 2, n, &out);
    if (rc) {
        snprintf(msg, 256, "%s", oracle_map_last_error(h));
        /* a failed call hands back no batch */
        CHECK(out.cols == NULL && out.n_rows == 0);
    } else {
        CHECK(out.n_rows == n && out.n_cols == 1);
        memcpy(got, out.cols[0], (size_t)n * 8);
        oracle_free_out(&out);
    }
    oracle_map_destroy(h);
    return rc;
}

static void wrapping_corners(void) {
    const int64_t a[4] = {INT64_MAX, INT64_MIN, INT64_MIN, INT64_MAX};
    const int64_t b[4] = {1, -1, INT64_MIN, INT64_MAX};
    int64_t got[4];
    char msg[256];
    CHECK(run(AMD_MOP_ADD, a, b, 4, got, msg) == 0);
    CHECK(got[0] == INT64_MIN && got[1] == INT64_MAX && got[2] == 0 &&
          got[3] == -2);
    CHECK(run(AMD_MOP_SUB, a, b, 4, got, msg) == 0);
    CHECK(got[0] == INT64_MAX - 1 && got[1] == INT64_MIN + 1 && got[2] == 0 &&
          got[3] == 0);
    const int64_t s[4] = {-1, INT64_MAX, INT64_MIN, 1};
    CHECK(run(AMD_MOP_SUB, s, a, 4, got, msg) == 0);
    CHECK(got[0] == INT64_MIN && got[1] == -1 && got[2] == 0 &&
          got[3] == INT64_MIN + 2);
    CHECK(run(AMD_MOP_MUL, a, b, 4, got, msg) == 0);
    CHECK(got[0] == INT64_MAX && got[1] == INT64_MIN && got[2] == 0 &&
          got[3] == 1);
}

static void min_by_minus_one(void) {
    const int64_t a[3] = {7, INT64_MIN, -7}, b[3] = {2, -1, 2};
    int64_t got[3];
    char msg[256] = "";
    CHECK(run(AMD_MOP_DIV, a, b, 3, got, msg) == 1);
    CHECK(strstr(msg, "overflow") != NULL);
    CHECK(run(AMD_MOP_MOD, a, b, 3, got, msg) == 0);
    CHECK(got[0] == 1 && got[1] == 0 && got[2] == -1);
    CHECK(run(AMD_MOP_DIV, a, b, 1, got, msg) == 0 && got[0] == 3);
}

static void f2i_out_of_range(void) {
    const double bad[] = {NAN, INFINITY, -INFINITY, 0x1p63, 1e19, -1e19,
                          -0x1.0000000000001p63, 1.7976931348623157e308,
                          -1.7976931348623157e308};
    const int64_t zero[2] = {0, 0};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
        const int64_t a[2] = {bits(1.5), bits(bad[i])};
        int64_t got[2];
        char msg[256] = "";
        CHECK(run(AMD_MOP_F2I, a, zero, 2, got, msg) == 1);
        CHECK(strstr(msg, "cast") != NULL);
    }
    const int64_t ok[4] = {bits(-0x1p63), bits(0x1.fffffffffffffp62),
                           bits(-0.0), bits(-1.5)};
    const int64_t z4[4] = {0, 0, 0, 0};
    int64_t got[4];
    char msg[256];
    CHECK(run(AMD_MOP_F2I, ok, z4, 4, got, msg) == 0);
    CHECK(got[0] == INT64_MIN && got[1] == INT64_MAX - 1023 && got[2] == 0 &&
          got[3] == -1);
}

static void division_by_zero_then_recovery(void) {
    AmdMapConfig c = binary(AMD_MOP_DIV);
    void *h = oracle_map_create(&c);
    CHECK(h != NULL);
    if (!h) return;
    const int64_t a[3] = {6, 7, 8}, b[3] = {3, 0, 2}, b2[3] = {3, 7, 2};
    const int64_t *cols[2] = {a, b}, *cols2[2] = {a, b2};
    AmdOutBatch out;
    /* the batch allocated before the failing row must not leak */
    CHECK(oracle_map_process_batch(h, cols, 2, 3, &out) == 1);
    CHECK(strstr(oracle_map_last_error(h), "division by zero") != NULL);
    CHECK(out.cols == NULL);
    CHECK(oracle_map_process_batch(h, cols2, 2, 3, &out) == 0);
    CHECK(out.n_rows == 3 && ((int64_t *)out.cols[0])[0] == 2 &&
          ((int64_t *)out.cols[0])[1] == 1 && ((int64_t *)out.cols[0])[2] == 4);
    oracle_free_out(&out);
    oracle_map_destroy(h);
}

static void rejected_configs(void) {
    AmdMapConfig c = binary(AMD_MOP_ADD);
    c.out_reg[0] = AMD_MAP_MAX_REGS;         /* used to index past regs[] */
    CHECK(oracle_map_create(&c) == NULL);
    CHECK(strstr(oracle_map_last_error(NULL), "invalid map") != NULL);
    c = binary(AMD_MOP_ADD);
    c.prog[0].a = 5;                         /* read before it is written */
    CHECK(oracle_map_create(&c) == NULL);
    c = binary(99);
    CHECK(oracle_map_create(&c) == NULL);
    c = binary(AMD_MOP_ADD);
    c.filter_reg = -7;
    CHECK(oracle_map_create(&c) == NULL);
    CHECK(oracle_map_create(NULL) == NULL);
}

int main(void) {
    wrapping_corners();
    min_by_minus_one();
    f2i_out_of_range();
    division_by_zero_then_recovery();
    rejected_configs();
    if (failures) {
        printf("map_oracle: %d check(s) failed\n", failures);
        return 1;
    }
    printf("map_oracle: ok\n");
    return 0;
}
