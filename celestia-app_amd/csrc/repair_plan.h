// repair_plan.h -- the host side of a batch repair (repair.hip,
// cda_repair_batch[_device], cda_repair_batch_plan): every decode sweep of
// every square, worked out before the first launch.  Plain C++ (no HIP
// headers), so a host compiler builds and tests it
// (tools/repair_plan_host_test.cpp).
//
// Which vectors become decodable in which sweep depends on the presence maps
// alone, never on the bytes.  The per-square rule is the fast path's of
// Engine::repair: in each iteration every incomplete row with >= k cells is
// decoded, then -- with the counts updated -- every such column, until
// nothing is decodable or every cell is present.
//
// The plan is one flat list of (square, axis, index) entries cut into
// segments in launch order: iteration 0 rows, iteration 0 columns, iteration
// 1 rows, ...  A segment holds the entries of all squares; empty segments are
// dropped.  A complete square and one with nothing decodable contribute no
// entries.
//
// Cost: the counts are kept incrementally -- a vector that completes bumps
// the orthogonal counts of the cells it filled -- so a square costs O(W^2)
// once, not per sweep.  The map is walked along rows wherever it can be: a
// column sweep of many columns is one pass over the rows under a column mask.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace cda {

// One codeword of a batch: axis 0 = row, 1 = column; index in the EDS of
// square `square`.  Also the device descriptor of the decode kernels.
struct RepairEntry {
    uint32_t square, axis, index;
};

struct RepairPlan {
    std::vector<RepairEntry> entries;
    std::vector<uint32_t> seg_off;    // n_segments + 1 offsets into entries
    std::vector<uint32_t> seg_sweep;  // per segment: 2 * iteration + axis
    std::vector<uint8_t> solved;      // per square: every cell present at the fixed point
    std::vector<uint8_t> complete;    // [n][2W]: vector axis * W + i complete at the fixed point
    uint32_t max_segment = 0;         // entries of the largest segment (sizes the error-locator scratch)
    uint32_t iterations = 0;          // iterations that decode something, the deepest square's
    uint32_t n_segments() const { return (uint32_t)seg_sweep.size(); }
};

// present: n maps of W x W bytes, any non-zero byte = present; W = 2k >= 2.
// normalised (optional): n * W * W bytes, the maps as 0 / 1.
inline void repair_plan(const uint8_t* present, uint32_t n, uint32_t W, RepairPlan* out,
                        uint8_t* normalised = nullptr) {
    const uint32_t k = W / 2;
    const size_t cells = (size_t)W * W;
    out->entries.clear();
    out->seg_off.assign(1, 0);
    out->seg_sweep.clear();
    out->solved.assign(n, 0);
    out->complete.assign((size_t)n * 2 * W, 0);
    out->max_segment = 0;
    out->iterations = 0;
    struct Tagged {
        uint32_t sweep;
        RepairEntry e;
    };
    std::vector<Tagged> found;          // square-major
    std::vector<uint32_t> per_sweep;    // entries per sweep tag
    std::vector<uint8_t> map(cells), mask(W);
    std::vector<uint32_t> cnt(2 * (size_t)W), todo;
    for (uint32_t sq = 0; sq < n; sq++) {
        const uint8_t* in = present + (size_t)sq * cells;
        uint8_t* p = map.data();
        uint32_t* rows = cnt.data();
        uint32_t* cols = cnt.data() + W;
        for (uint32_t c = 0; c < W; c++) cols[c] = 0;
        size_t held = 0;
        // row by row with local sums, so that both inner loops vectorise
        for (uint32_t r = 0; r < W; r++) {
            const uint8_t* src = in + (size_t)r * W;
            uint8_t* dst = p + (size_t)r * W;
            uint32_t sum = 0;
            for (uint32_t c = 0; c < W; c++) {
                const uint8_t v = src[c] != 0;
                dst[c] = v;
                sum += v;
            }
            for (uint32_t c = 0; c < W; c++) cols[c] += dst[c];
            rows[r] = sum;
            held += sum;
        }
        if (normalised) std::memcpy(normalised + (size_t)sq * cells, p, cells);
        for (uint32_t it = 0; held != cells; it++) {
            bool progress = false;
            for (uint32_t axis = 0; axis < 2; axis++) {
                uint32_t* mine = axis == 0 ? rows : cols;
                // decided on the counts as this axis' sweep starts: completing
                // a vector never changes the count of a parallel one
                todo.clear();
                for (uint32_t i = 0; i < W; i++)
                    if (mine[i] != W && mine[i] >= k) todo.push_back(i);
                if (todo.empty()) continue;
                if (axis == 0) {
                    for (uint32_t i : todo) {
                        uint8_t* row = p + (size_t)i * W;
                        for (uint32_t c = 0; c < W; c++) {
                            cols[c] += 1u - row[c];
                            row[c] = 1;
                        }
                        held += W - rows[i];
                    }
                } else if ((size_t)todo.size() * 8 >= W) {
                    // many columns: one contiguous pass over the map under a column mask (at most 16 such
                    // passes per square, since each completes >= W / 8 of the 2W vectors)
                    for (uint32_t c = 0; c < W; c++) mask[c] = 0;
                    for (uint32_t i : todo) mask[i] = 1;
                    for (uint32_t r = 0; r < W; r++) {
                        uint8_t* row = p + (size_t)r * W;
                        uint32_t add = 0;
                        for (uint32_t c = 0; c < W; c++) {
                            add += mask[c] & (row[c] ^ 1);
                            row[c] |= mask[c];
                        }
                        rows[r] += add;
                        held += add;
                    }
                } else {
                    for (uint32_t i : todo)
                        for (uint32_t r = 0; r < W; r++) {
                            uint8_t& cell = p[(size_t)r * W + i];
                            rows[r] += 1u - cell;
                            held += 1u - cell;
                            cell = 1;
                        }
                }
                const uint32_t sweep = 2 * it + axis;
                if (per_sweep.size() <= sweep) per_sweep.resize(sweep + 1, 0);
                per_sweep[sweep] += (uint32_t)todo.size();
                for (uint32_t i : todo) {
                    mine[i] = W;
                    found.push_back(Tagged{sweep, RepairEntry{sq, axis, i}});
                }
                progress = true;
            }
            if (!progress) break;
            if (it + 1 > out->iterations) out->iterations = it + 1;
        }
        out->solved[sq] = held == cells;
        for (uint32_t i = 0; i < 2 * W; i++) out->complete[(size_t)sq * 2 * W + i] = cnt[i] == W;
    }
    // segments in launch order; the squares stay in order inside each
    std::vector<uint32_t> at(per_sweep.size(), 0);
    uint32_t total = 0;
    for (uint32_t t = 0; t < per_sweep.size(); t++) {
        at[t] = total;
        if (per_sweep[t] == 0) continue;
        total += per_sweep[t];
        out->seg_off.push_back(total);
        out->seg_sweep.push_back(t);
        if (per_sweep[t] > out->max_segment) out->max_segment = per_sweep[t];
    }
    out->entries.resize(total);
    for (const Tagged& f : found) out->entries[at[f.sweep]++] = f.e;
}

}  // namespace cda
