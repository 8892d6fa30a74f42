// push_order.h -- the push-order word: a square's first nmt ErrInvalidPushOrder
// violation in one u32.  Plain C++ (host and device, and a CPU test:
// tools/push_order_host_test.cpp); the one home of the layout.
//
//   axis << 24 | index << 12 | pos      kOrdered (~0) = no violation
// axis 0 = row tree, 1 = column tree; index = which row / column (< 4096);
// pos = push position of the out-of-order leaf (1 .. 4095).  Rows sort below
// columns, then lower index, then lower position, so the minimum of a square's
// violation words (atomicMin on the device) is the violation the reference,
// which pushes row trees first, reports.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace cda::push_order {

constexpr uint32_t kOrdered = 0xFFFFFFFFu;
constexpr uint32_t kAxisShift = 24, kIndexShift = 12, kFieldMask = 0xFFF;

constexpr uint32_t encode(uint32_t axis, uint32_t index, uint32_t pos) {
    return (axis << kAxisShift) | (index << kIndexShift) | pos;
}

struct Violation {
    int32_t axis;   // -1: ordered
    uint32_t index, pos;
};
constexpr Violation decode(uint32_t word) {
    if (word == kOrdered) return {-1, 0, 0};
    return {(int32_t)(word >> kAxisShift), (word >> kIndexShift) & kFieldMask, word & kFieldMask};
}

// Per-square status of n words (status may be NULL).  The two values are
// CDA_OK / CDA_ERR_PUSH_ORDER of include/cda.h (engine.hip asserts it).
constexpr int32_t kStatusOk = 0, kStatusViolation = -3;
inline void fill_status(const uint32_t* words, size_t n, int32_t* status) {
    if (!status) return;
    for (size_t i = 0; i < n; i++) status[i] = words[i] == kOrdered ? kStatusOk : kStatusViolation;
}

}  // namespace cda::push_order
