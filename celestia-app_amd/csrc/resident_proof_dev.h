// resident_proof_dev.h -- what the kernels that serve proofs from a resident
// square share (sample.hip, share_proofs.hip): the read-only view of the
// square, the staging of 96-byte node slots into a wave's LDS row, the wave's
// store of packed items (90-byte nodes, 29-byte namespaces) from that row, and
// the merkle proof of a row or column root against the data root.  The helpers
// take `lane`; every branch in them is uniform over the wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha256_dev.h"

namespace cda {

constexpr uint32_t kProofMaxD = 11;            // log2(2 * 1024): the deepest axis tree
constexpr uint32_t kSlotPieces = kSlot / 16;   // 16-byte loads per slot

// uint4 entries of a wave's LDS stage row that holds `slots` slots.
constexpr uint32_t stage_row(uint32_t slots) { return slots * kSlotPieces; }

// What the proof kernels read of a resident square (ResidentSquare::view()).
struct ResidentView {
    const uint8_t* eds;         // [W][W][512]
    const uint8_t* levels;      // row levels, level 0 = the leaf slots
    const uint8_t* col_levels;  // column levels 1..
    const uint8_t* root_slots;  // [2W][96]: row roots, then column roots
    const uint32_t* rfc;        // RFC-6962 levels of the data-root tree, state words
    uint32_t k, log_w;
};

// Per-square strides of a set's arenas (square_set.hip), bytes; unused for a single square.
struct SetStrides {
    uint64_t eds, levels, col_levels, root_slots, rfc;
};

// The view of square y of a set: `base` holds the arenas' bases.  y was validated on the host (below the
// set's square count); the offsets are 64-bit, an arena may be past 4 GiB.
__device__ __forceinline__ ResidentView member_view(const ResidentView& base, const SetStrides& sq, uint64_t y) {
    return ResidentView{base.eds + y * sq.eds, base.levels + y * sq.levels, base.col_levels + y * sq.col_levels,
                        base.root_slots + y * sq.root_slots,
                        reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(base.rfc) + y * sq.rfc),
                        base.k, base.log_w};
}

// Lane `lane`'s share of staging `count` slots into the row `st`, six 16-byte
// loads per slot: slot(n) gives the address of the n-th slot and the position
// in the row it goes to.
struct StagedSlot {
    const uint8_t* src;
    uint32_t at;
};
template <class F>
__device__ __forceinline__ void stage_slots(uint4* st, uint32_t count, uint32_t lane, F&& slot) {
    for (uint32_t q = lane; q < count * kSlotPieces; q += 64) {
        const uint32_t part = q % kSlotPieces;
        const StagedSlot s = slot(q / kSlotPieces);
        st[s.at * kSlotPieces + part] = reinterpret_cast<const uint4*>(s.src)[part];
    }
}

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

// The merkle proof of root `idx` among the 2W roots rowRoots || colRoots
// (Total 4k), item i of the outputs: the leaf hash to leaf_hash[32 i ..) and
// the A = log2(2W) aunts, bottom-up, to aunts[32 A i ..), from the retained
// RFC levels (level l starts at entry 2T - (2T >> l), T = 2W): state words out
// as big-endian bytes, one word per lane.  Either output may be NULL.
__device__ __forceinline__ void store_root_proof(const uint32_t* rfc, uint32_t W, uint32_t A, uint32_t idx, uint64_t i,
                                                 uint8_t* leaf_hash, uint8_t* aunts, uint32_t lane) {
    const uint32_t T = 2 * W;
    for (uint32_t q = lane; q < (A + 1) * 8; q += 64) {
        const uint32_t item = q / 8, word = q % 8;
        if (item == 0) {
            if (leaf_hash)
                reinterpret_cast<uint32_t*>(leaf_hash + i * 32)[word] = bswap32(rfc[(uint64_t)idx * 8 + word]);
        } else if (aunts) {
            const uint32_t l = item - 1;
            const uint64_t entry = (uint64_t)(2 * T - ((2 * T) >> l)) + ((idx >> l) ^ 1u);
            reinterpret_cast<uint32_t*>(aunts + (i * A + l) * 32)[word] = bswap32(rfc[entry * 8 + word]);
        }
    }
}

}  // namespace cda
