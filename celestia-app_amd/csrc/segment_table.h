// segment_table.h -- the segment table that drives the proof kernel of a
// resident square (share_proofs.hip) and what its two producers hand to the
// one body that uploads the table, launches the kernel and copies the outputs
// back (Engine::emit_segments): the share-range proofs (share_proofs.hip) and
// the namespace proofs (namespace_proofs.hip); the blob commitment proofs
// (share_proofs.hip) are a third segment kind.  Plain C++ (no HIP headers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cda {

constexpr uint32_t kUnitShares = 16;   // shares one wave copies

// One segment (one leaf range of one row tree), as uploaded: 32 bytes.
struct SegEntry {
    uint32_t row;          // seg_row_word: the row, and above it the square of a set (0 for a single square)
    uint32_t range;        // s0 | e0 << 16: the leaf range in the row tree; kSegAbsence: no shares, the leaf s0 itself
    uint32_t node_off;     // first node of the segment in `nodes`
    uint32_t unit_off;     // first share unit of the segment; kSegSubtree: log2 of the blob's subtree width
    uint64_t share_off;    // first share of the segment in `shares`; kSegSubtree: first root in `subtree_roots`
    uint32_t proof;
    uint32_t first_cell;   // EDS cell (row * W + col) of the proof's first share; kNoFirstCell: no namespace output
};
static_assert(sizeof(SegEntry) == 32);
constexpr uint32_t kSegAbsence = 1u << 31;
constexpr uint32_t kSegSubtree = 1u << 30;   // no shares: the subtree roots of [s0, e0) (commitment_proofs_plan.h)
constexpr uint32_t kSegEndMask = 0xFFFu;   // e0 <= 2048
constexpr uint32_t kNoFirstCell = 0xFFFFFFFFu;
constexpr uint32_t kSegWords = sizeof(SegEntry) / 4;

// The `row` word.  Rows are below 2048 (2k <= 2048) and a set holds at most 65 535 squares
// (CDA_SET_MAX_SQUARES), so the square a segment is served from lies beside its row: the row in the low half,
// the square in the high half.  A single square's table has square 0: its word is the row itself.
constexpr uint32_t kSegRowBits = 16, kSegRowMask = (1u << kSegRowBits) - 1, kSegMaxSquares = 65535;
constexpr uint32_t seg_row_word(uint32_t row, uint32_t square) { return row | (square << kSegRowBits); }
constexpr uint32_t seg_row(uint32_t word) { return word & kSegRowMask; }
constexpr uint32_t seg_square(uint32_t word) { return word >> kSegRowBits; }

constexpr uint32_t seg_units(uint32_t shares) { return (shares + kUnitShares - 1) / kUnitShares; }

// A filled table and the caller's host buffers (NULL: not requested) with their sizes.
struct SegmentEmit {
    std::vector<uint32_t> up;   // n_segs entries, then n_flags one_namespace bytes preset to 1, padded to words,
                                // then (commitments) the n_flags + 1 first roots of the proofs
    uint32_t n_segs = 0, n_units = 0, n_flags = 0;
    size_t node_slots = 0, n_aunts = 0;
    uint64_t n_shares = 0;
    uint8_t* nodes = nullptr;           // node_slots * 90
    uint8_t* row_roots = nullptr;       // n_segs * 90
    uint8_t* leaf_hash = nullptr;       // n_segs * 32
    uint8_t* aunts = nullptr;           // n_aunts * 32
    uint8_t* shares = nullptr;          // n_shares * 512
    uint8_t* namespaces = nullptr;      // n_flags * 29
    uint8_t* one_namespace = nullptr;   // n_flags
    uint8_t* absence_leaf = nullptr;    // n_segs * 90: the leaf of an absence segment, zero for the others
    // a table of kSegSubtree segments only (commitment proofs)
    size_t n_roots = 0;
    uint32_t max_roots = 0;             // the most subtree roots of one proof
    uint8_t* subtree_roots = nullptr;   // n_roots * 90
    uint8_t* commitments = nullptr;     // n_flags * 32: the RFC-6962 root of each proof's subtree roots
    int stage = -1;                     // Engine::Stage that brackets every launch of the call; -1: none
    size_t one_copy_max = 0;            // outputs up to this size return in one copy
    SegEntry* segs() { return reinterpret_cast<SegEntry*>(up.data()); }
};

}  // namespace cda
