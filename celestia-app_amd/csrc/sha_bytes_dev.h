// sha_bytes_dev.h -- byte-addressed SHA-256 and namespace loading for the
// generic paths (any cell length, any namespace length): tree.hip's generic
// trees and RFC-6962 roots, verify.hip's byte nodes.  The square-shaped sizes
// run on the word-level builders of sha256_dev.h / leaf_dev.h instead.
#pragma once
#include "sha256_dev.h"

namespace cda {

// SHA-256 of tag || a[0:na] || b[0:nb] (any lengths, any addresses; a pointer
// whose length is 0 is not read), big-endian state words.
__device__ inline void sha_cat(uint32_t tag, const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb,
                               uint32_t (&out)[8]) {
    ShaState st;
    sha_init(st);
    const uint64_t total = 1 + na + nb;
    const uint64_t n_blocks = (total + 9 + 63) / 64;
    const uint64_t bits = total * 8;
    auto byte_at = [&](uint64_t i) -> uint32_t {
        if (i == 0) return tag;
        if (i <= na) return a[i - 1];
        if (i < total) return b[i - 1 - na];
        if (i == total) return 0x80u;
        return 0;
    };
#pragma unroll 1
    for (uint64_t blk = 0; blk < n_blocks; blk++) {
        uint32_t w[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t p = blk * 64 + 4 * j;
            w[j] = (byte_at(p) << 24) | (byte_at(p + 1) << 16) | (byte_at(p + 2) << 8) | byte_at(p + 3);
        }
        if (blk == n_blocks - 1) {
            w[14] = (uint32_t)(bits >> 32);
            w[15] = (uint32_t)bits;
        }
        sha_compress(st, w);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) out[j] = st.h[j];
}

// Big-endian namespace words (byte 28 in the top byte of word 7, the rest of
// it zero) from 29 bytes at any address; parity: ParitySharesNamespace
// (29 x 0xFF) and p is not read.
__device__ __forceinline__ void load_ns_bytes(const uint8_t* p, bool parity, uint32_t (&ns)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (4 * j + q < kNs) v |= (parity ? 0xFFu : (uint32_t)p[4 * j + q]) << (24 - 8 * q);
        ns[j] = v;
    }
}

}  // namespace cda
