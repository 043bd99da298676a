/* Host side of AmdOutBatch: allocation and release of the callee-allocated
 * output batch every operator returns.  Plain C++ (no HIP), so it is also
 * compiled on its own under sanitizers (tests/op_out_main.cpp). */
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../include/arroyo_amd_types.h"

/* free a host-resident batch and zero it; a zeroed batch is a no-op */
inline void out_free_host(AmdOutBatch *out) {
    if (!out) return;
    for (int i = 0; out->cols && i < out->n_cols; i++) free(out->cols[i]);
    for (int i = 0; out->validity && i < out->n_cols; i++)
        free(out->validity[i]);
    free(out->validity);
    free(out->cols);
    free(out->is_f64);
    memset(out, 0, sizeof *out);
}

/* n_cols host columns of n_rows 8-byte elements (at least one element each,
 * so a column pointer is never NULL), is_f64 all zero.  Nonzero on
 * allocation failure, with everything taken freed and *out zeroed. */
inline int out_alloc(AmdOutBatch *out, int64_t n_rows, int n_cols) {
    memset(out, 0, sizeof *out);
    if (n_rows < 0 || n_cols < 0 || (uint64_t)n_rows > SIZE_MAX / 8) return 1;
    out->n_rows = n_rows;
    out->n_cols = n_cols;
    out->cols = (void **)calloc(n_cols ? n_cols : 1, sizeof(void *));
    out->is_f64 = (int32_t *)calloc(n_cols ? n_cols : 1, sizeof(int32_t));
    bool ok = out->cols && out->is_f64;
    for (int i = 0; ok && i < n_cols; i++)
        ok = (out->cols[i] = malloc((size_t)(n_rows ? n_rows : 1) * 8));
    if (!ok) out_free_host(out);
    return !ok;
}

/* the validity pointer table of an allocated batch: every column all-valid
 * (NULL) until out_validity_col gives it a bitmap */
inline int out_alloc_validity(AmdOutBatch *out) {
    out->validity =
        (uint8_t **)calloc(out->n_cols ? out->n_cols : 1, sizeof(uint8_t *));
    return !out->validity;
}

/* zeroed Arrow bitmap ((n_rows + 7) / 8 bytes) for column c; NULL on
 * allocation failure */
inline uint8_t *out_validity_col(AmdOutBatch *out, int c) {
    size_t nbytes = (size_t)((out->n_rows + 7) / 8);
    free(out->validity[c]);
    return out->validity[c] = (uint8_t *)calloc(nbytes ? nbytes : 1, 1);
}

/* Append the first n_bits bits of the Arrow bitmap `src` (bit offset 0; its
 * bits past n_bits may hold anything) to `dst` at bit offset dst_bit;
 * src == nullptr appends n_bits ones.  `dst` is a bitmap filled front to
 * back: its bits from dst_bit on are clear on entry, and those from
 * dst_bit + n_bits on are still clear on return.  It must hold
 * (dst_bit + n_bits + 7) / 8 bytes; no byte past that is touched.  This is
 * how a filtered operator joins the bitmaps of its chunks, whose kept counts
 * are no multiple of 8. */
inline void out_validity_append_bits(uint8_t *dst, int64_t dst_bit,
                                     const uint8_t *src, int64_t n_bits) {
    if (n_bits <= 0) return;
    unsigned sh = (unsigned)(dst_bit & 7);
    uint8_t *d = dst + (dst_bit >> 3);
    int64_t n_bytes = (n_bits + 7) >> 3;
    unsigned tail = (unsigned)(n_bits & 7);
    for (int64_t i = 0; i < n_bytes; i++) {
        unsigned b = src ? src[i] : 0xffu;
        if (tail && i == n_bytes - 1) b &= (1u << tail) - 1u;
        d[i] |= (uint8_t)(b << sh);
        /* a nonzero carry lies below dst_bit + n_bits: that byte exists */
        unsigned carry = b >> (8 - sh);
        if (carry) d[i + 1] |= (uint8_t)carry;
    }
}
