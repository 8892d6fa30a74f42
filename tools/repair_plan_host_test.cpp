// repair_plan_host_test.cpp -- stand-alone driver of csrc/repair_plan.h (host
// only; tests/test_repair_batch_plan.py builds it with g++, once more with
// -fsanitize=address,undefined).
//
//   repair_plan_host_test W n FILE
//     FILE: n presence maps of W x W bytes (any non-zero byte = present).
//     Prints
//       S <segments> <iterations> <max_segment> <entries>
//       G <2 * iteration + axis> : <square>:<axis>:<index> ...     per segment, launch order
//       Q <square> <solved> <2W digits: vector axis * W + i complete at the fixed point>
//   repair_plan_host_test
//     A self-check: seeded random batches of every width up to 64 against a
//     closure computed here without the incremental counts; prints "OK <maps>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "repair_plan.h"

namespace {

void print_plan(const cda::RepairPlan& p, uint32_t n, uint32_t W) {
    printf("S %u %u %u %zu\n", p.n_segments(), p.iterations, p.max_segment, p.entries.size());
    for (uint32_t g = 0; g < p.n_segments(); g++) {
        printf("G %u :", p.seg_sweep[g]);
        for (uint32_t i = p.seg_off[g]; i < p.seg_off[g + 1]; i++)
            printf(" %u:%u:%u", p.entries[i].square, p.entries[i].axis, p.entries[i].index);
        printf("\n");
    }
    for (uint32_t q = 0; q < n; q++) {
        printf("Q %u %u ", q, (unsigned)p.solved[q]);
        for (uint32_t i = 0; i < 2 * W; i++) putchar('0' + p.complete[(size_t)q * 2 * W + i]);
        printf("\n");
    }
}

// "a vector with >= k cells becomes full" until nothing changes, counting from scratch every time
std::vector<uint8_t> closure(const uint8_t* in, uint32_t W) {
    const uint32_t k = W / 2;
    std::vector<uint8_t> p((size_t)W * W);
    for (size_t i = 0; i < p.size(); i++) p[i] = in[i] ? 1 : 0;
    for (bool changed = true; changed;) {
        changed = false;
        for (uint32_t axis = 0; axis < 2; axis++)
            for (uint32_t i = 0; i < W; i++) {
                uint32_t c = 0;
                for (uint32_t o = 0; o < W; o++) c += p[axis == 0 ? (size_t)i * W + o : (size_t)o * W + i];
                if (c == W || c < k) continue;
                for (uint32_t o = 0; o < W; o++) p[axis == 0 ? (size_t)i * W + o : (size_t)o * W + i] = 1;
                changed = true;
            }
    }
    return p;
}

int self_check() {
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return state;
    };
    unsigned maps = 0;
    for (uint32_t W = 2; W <= 64; W *= 2)
        for (uint32_t density = 1; density <= 9; density++) {
            const uint32_t n = 5;
            const size_t cells = (size_t)W * W;
            std::vector<uint8_t> present(n * cells), norm(n * cells);
            for (auto& v : present) v = next() % 10 < density ? (uint8_t)(1 + next() % 255) : 0;
            cda::RepairPlan p;
            cda::repair_plan(present.data(), n, W, &p, norm.data());
            std::vector<uint8_t> seen((size_t)n * 2 * W, 0);
            for (const cda::RepairEntry& e : p.entries) {
                if (e.square >= n || e.axis > 1 || e.index >= W || seen[((size_t)e.square * 2 + e.axis) * W + e.index]++) {
                    fprintf(stderr, "bad or repeated entry at W=%u density=%u\n", W, density);
                    return 1;
                }
            }
            for (uint32_t q = 0; q < n; q++) {
                const std::vector<uint8_t> fix = closure(&present[q * cells], W);
                bool all = true;
                for (uint8_t v : fix) all = all && v;
                if (all != (p.solved[q] != 0)) {
                    fprintf(stderr, "solved differs at W=%u density=%u square %u\n", W, density, q);
                    return 1;
                }
                for (uint32_t a = 0; a < 2 * W; a++) {
                    const uint32_t axis = a / W, i = a % W;
                    uint32_t before = 0, after = 0;
                    for (uint32_t o = 0; o < W; o++) {
                        const size_t c = axis == 0 ? (size_t)i * W + o : (size_t)o * W + i;
                        before += norm[q * cells + c];
                        after += fix[c];
                    }
                    // planned = completed by a decode; a vector other decodes filled cell by cell is planned
                    // only if it reached k cells before it was full, which the closure cannot tell: skip those
                    const bool planned = seen[((size_t)q * 2 + axis) * W + i] != 0;
                    if ((after == W) != (p.complete[(size_t)q * 2 * W + a] != 0) || (planned && (before == W || after != W))) {
                        fprintf(stderr, "vector differs at W=%u density=%u square %u vector %u\n", W, density, q, a);
                        return 1;
                    }
                }
                maps++;
            }
        }
    printf("OK %u\n", maps);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 1) return self_check();
    if (argc != 4) {
        fprintf(stderr, "usage: %s [W n FILE]\n", argv[0]);
        return 2;
    }
    const uint32_t W = (uint32_t)strtoul(argv[1], nullptr, 10), n = (uint32_t)strtoul(argv[2], nullptr, 10);
    if (W < 2 || (W & (W - 1)) || W > 1024) {
        fprintf(stderr, "EDS width must be a power of two in [2, 1024]\n");
        return 2;
    }
    std::vector<uint8_t> present((size_t)n * W * W);
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(present.data(), 1, present.size(), f) != present.size()) {
        fprintf(stderr, "cannot read %zu bytes from %s\n", present.size(), argv[3]);
        if (f) fclose(f);
        return 2;
    }
    fclose(f);
    cda::RepairPlan p;
    cda::repair_plan(present.data(), n, W, &p);
    print_plan(p, n, W);
    return 0;
}
