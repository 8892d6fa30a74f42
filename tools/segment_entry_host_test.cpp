// segment_entry_host_test.cpp -- the `row` word of a segment table entry
// (csrc/segment_table.h: seg_row_word / seg_row / seg_square), host only.
// Prints one "name : values" line per case; tests/test_segment_entry.py
// compares the lines with values worked out by hand.
//   g++ -O2 -std=c++20 -I celestia-app_amd/csrc tools/segment_entry_host_test.cpp -o segment_entry_host_test
#include <cstdio>
#include <cstring>

#include "segment_table.h"

using namespace cda;

static void round_trip(uint32_t row, uint32_t square) {
    const uint32_t w = seg_row_word(row, square);
    std::printf("W %u %u : %u %u %u\n", row, square, w, seg_row(w), seg_square(w));
}

int main() {
    std::printf("S size : %zu %u\n", sizeof(SegEntry), kSegWords);
    for (uint32_t row : {0u, 1u, 2047u})
        for (uint32_t square : {0u, 1u, 65534u}) round_trip(row, square);
    // An entry as the producers fill it, with each flag of the range word: the row word and the range word do
    // not disturb each other, and the entry's bytes are the eight little-endian words in order.
    for (uint32_t flag : {0u, kSegAbsence, kSegSubtree}) {
        SegEntry e{seg_row_word(2047, 65534), 5u | (9u << 16) | flag, 7, 11, 0x123456789ull, 13, kNoFirstCell};
        uint32_t w[kSegWords];
        std::memcpy(w, &e, sizeof(e));
        std::printf("E %u :", flag >> 30);
        for (uint32_t x : w) std::printf(" %u", x);
        std::printf(" | %u %u %u %u %u %u\n", seg_row(e.row), seg_square(e.row), e.range & 0xFFFFu,
                    (e.range >> 16) & kSegEndMask, (e.range & kSegAbsence) != 0, (e.range & kSegSubtree) != 0);
    }
    // a single square's word is the row itself
    std::printf("Z single : %u %u\n", seg_row_word(77, 0), seg_row_word(2047, 0));
    std::printf("M max : %u %u\n", kSegMaxSquares, seg_square(seg_row_word(2047, kSegMaxSquares - 1)));
    return 0;
}
