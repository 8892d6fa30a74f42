// out_regions.h -- where the outputs of one call lie in a resident square's
// scratch buffer (sample.hip, share_proofs.hip): the call's upload, then one
// region per requested host output, each at a 16-byte boundary.  Plain C++ (no
// HIP headers: tools/out_regions_host_test.cpp); the Engine makes the copies.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cda {

class OutRegions {
  public:
    struct Region {
        uint8_t* host;       // NULL: not requested
        size_t off, bytes;   // in the scratch buffer; bytes is 0 when host is NULL
        // The kernel's pointer for this output: NULL when it was not requested.
        uint8_t* dev(uint8_t* scratch) const { return host ? scratch + off : nullptr; }
    };
    struct Span {   // [off, off + bytes) of the scratch buffer
        size_t off, bytes;
    };
    static constexpr size_t align(size_t n) { return (n + 15) & ~(size_t)15; }

    explicit OutRegions(size_t upload_bytes) : total_(align(upload_bytes)) {}
    // The next region behind everything laid out so far.
    Region add(void* host, size_t bytes) {
        const Region r = add_at(host, total_, bytes);
        total_ += align(r.bytes);
        return r;
    }
    // A region at byte `off`: one the upload itself holds (an output that starts from uploaded values).
    Region add_at(void* host, size_t off, size_t bytes) {
        const Region r{static_cast<uint8_t*>(host), off, host ? bytes : 0};
        if (r.bytes) copies_.push_back(r);
        return r;
    }
    size_t total() const { return total_; }   // bytes of scratch the call needs
    // The regions to copy out (the requested ones of non-zero size), in the order added.
    const std::vector<Region>& copies() const { return copies_; }
    // The one span that covers every region to copy out; {0, 0} if there is none.
    Span span() const {
        if (copies_.empty()) return Span{0, 0};
        size_t lo = copies_[0].off, hi = lo;
        for (const Region& r : copies_) {
            if (r.off < lo) lo = r.off;
            if (r.off + r.bytes > hi) hi = r.off + r.bytes;
        }
        return Span{lo, hi - lo};
    }

  private:
    size_t total_;
    std::vector<Region> copies_;
};

}  // namespace cda
