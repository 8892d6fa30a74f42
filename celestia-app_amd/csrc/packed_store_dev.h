// packed_store_dev.h -- the wave's store of packed items (90-byte nodes,
// 29-byte namespaces) that start at any byte address, shared by the proof
// kernels that serve them from LDS (sample.hip, share_proofs.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha256_dev.h"

namespace cda {

// `count` items of ITEM bytes, held in LDS at a stride of kSlot bytes, to the
// packed bytes dst[0 : count * ITEM) at any address: whole aligned words by one
// 4-byte store per lane, the bytes of a word that the region only partly covers
// singly (a neighbouring item's owner has the rest of that word).
template <uint32_t ITEM>
__device__ __forceinline__ void store_packed(const uint8_t* lds, uint32_t count, uint8_t* dst, uint32_t lane) {
    const uint32_t len = count * ITEM;
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
    const uint32_t n_words = (a + len + 3) / 4;
    for (uint32_t w = lane; w < n_words; w += 64) {
        const int32_t b0 = (int32_t)(4 * w) - (int32_t)a;
        uint32_t v = 0;
        bool full = true;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int32_t b = b0 + t;
            if (b >= 0 && b < (int32_t)len) {
                const uint32_t item = (uint32_t)b / ITEM, o = (uint32_t)b % ITEM;
                v |= (uint32_t)lds[item * kSlot + o] << (8 * t);
            } else {
                full = false;
            }
        }
        if (full) {
            *reinterpret_cast<uint32_t*>(dst + b0) = v;
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int32_t b = b0 + t;
                if (b >= 0 && b < (int32_t)len) dst[b] = (uint8_t)(v >> (8 * t));
            }
        }
    }
}

}  // namespace cda
