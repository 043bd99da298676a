/* Stand-alone exerciser of out_validity_append_bits
 * (arroyo_amd/csrc/op_out.h), built by tests/test_op_out_bits_host.py with
 * -fsanitize=address,undefined and run as a child process.  Every buffer is
 * a heap block of exactly the bytes the contract names, so one byte read or
 * written past either end is an ASan report.  Exits 0 when every check
 * holds. */
#include <cstdio>
#include <vector>

#include "../arroyo_amd/csrc/op_out.h"

static int failures;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__,  \
                    #cond);                                                   \
            failures++;                                                       \
        }                                                                     \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static unsigned rnd() {             /* xorshift64 */
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

static bool get_bit(const uint8_t *bm, int64_t i) {
    return bm[i >> 3] >> (i & 7) & 1;
}
static void set_bit(uint8_t *bm, int64_t i) {
    bm[i >> 3] |= (uint8_t)(1u << (i & 7));
}

/* a heap block of exactly n bytes (n may be 0: a valid, unreadable block) */
struct Block {
    uint8_t *p;
    size_t n;
    explicit Block(size_t bytes) : p((uint8_t *)malloc(bytes)), n(bytes) {
        if (n) memset(p, 0, n);
    }
    ~Block() { free(p); }
};

/* one append at bit offset `off` of `len` bits; ones: src == nullptr */
static void one_case(int64_t off, int64_t len, bool ones) {
    size_t dst_bytes = (size_t)((off + len + 7) / 8);
    Block dst(dst_bytes), want(dst_bytes), src((size_t)((len + 7) / 8));
    /* what earlier appends left: `off` bits of anything, clear from there */
    for (int64_t i = 0; i < off; i++)
        if (rnd() & 1) {
            set_bit(dst.p, i);
            set_bit(want.p, i);
        }
    /* the source: `len` bits of anything, then a dirty tail of ones */
    for (int64_t i = 0; i < (int64_t)src.n * 8; i++)
        if (i >= len || (rnd() & 1)) set_bit(src.p, i);
    /* the reference: one bit at a time */
    for (int64_t i = 0; i < len; i++)
        if (ones || get_bit(src.p, i)) set_bit(want.p, off + i);
    out_validity_append_bits(dst.p, off, ones ? nullptr : src.p, len);
    bool same = dst_bytes == 0 || memcmp(dst.p, want.p, dst_bytes) == 0;
    if (!same)
        fprintf(stderr, "off %lld len %lld ones %d differs\n", (long long)off,
                (long long)len, (int)ones);
    CHECK(same);
    /* bits past the end are clear (the dirty source tail did not leak) */
    for (int64_t i = off + len; i < (int64_t)dst_bytes * 8; i++)
        CHECK(!get_bit(dst.p, i));
}

/* a bitmap built the way a chunked, filtered operator builds it: appends of
 * uneven lengths back to back, against the concatenation bit by bit */
static void chained(const std::vector<int64_t> &lens) {
    int64_t total = 0;
    for (int64_t l : lens) total += l;
    Block dst((size_t)((total + 7) / 8)), want((size_t)((total + 7) / 8));
    int64_t at = 0;
    for (int64_t l : lens) {
        Block src((size_t)((l + 7) / 8));
        for (int64_t i = 0; i < (int64_t)src.n * 8; i++)
            if (i >= l || (rnd() & 1)) set_bit(src.p, i);
        for (int64_t i = 0; i < l; i++)
            if (get_bit(src.p, i)) set_bit(want.p, at + i);
        out_validity_append_bits(dst.p, at, src.p, l);
        at += l;
    }
    CHECK(dst.n == 0 || memcmp(dst.p, want.p, dst.n) == 0);
}

int main() {
    const int64_t lens[] = {0, 1, 7, 8, 9, 63, 64, 65};
    int cases = 0;
    for (int64_t off = 0; off <= 15; off++)
        for (int64_t len : lens)
            for (int ones = 0; ones < 2; ones++) {
                one_case(off, len, ones != 0);
                cases++;
            }
    CHECK(cases == 16 * 8 * 2);
    /* a negative length is nothing, like a zero one */
    out_validity_append_bits(nullptr, 3, nullptr, 0);
    out_validity_append_bits(nullptr, 3, nullptr, -5);
    chained({3, 0, 5, 8, 1, 63, 65, 7, 64, 9});
    chained({699051, 699050, 3});   /* two filtered 2^20-row chunks' worth */
    chained({0});
    if (failures) return 1;
    puts("op_out_bits: ok");
    return 0;
}
