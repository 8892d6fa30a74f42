// Host dump and self-check of csrc/out_regions.h (where the outputs of a
// resident-square call lie in its scratch buffer), for
// tests/test_out_regions.py.  Build: g++ -std=c++20 -I celestia-app_amd/csrc
// (plain host C++: also the program to build with -fsanitize=address,undefined).
//   L name : total span_off span_bytes | off bytes dev ...   one triple per region added; dev is the
//                                      region's offset from the scratch base, or -1 for a NULL pointer
//   C name : off bytes ...             the regions to copy out, in order
// Every layout is also checked here: regions aligned, disjoint, inside
// total(), behind the upload unless placed in it, the span covering exactly
// the copies, and the bytes that a copy of the span followed by memcpys
// delivers equal to those of one copy per region.  A difference is reported on
// stderr and fails the program.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "out_regions.h"

namespace {

int failures = 0;

void fail(const char* name, const char* what) {
    fprintf(stderr, "%s: %s\n", name, what);
    failures++;
}

struct Ask {
    bool host;       // a host buffer is given
    size_t bytes;
    long in_upload;  // >= 0: the region lies at this byte of the upload
};

void layout_line(const char* name, size_t upload, const std::vector<Ask>& asks) {
    cda::OutRegions out(upload);
    std::vector<std::vector<uint8_t>> host(asks.size());
    std::vector<cda::OutRegions::Region> regs;
    for (size_t i = 0; i < asks.size(); i++) {
        host[i].assign(asks[i].bytes + 1, 0xAA);   // + 1: a zero-byte request still has a pointer
        void* h = asks[i].host ? host[i].data() : nullptr;
        regs.push_back(asks[i].in_upload >= 0 ? out.add_at(h, (size_t)asks[i].in_upload, asks[i].bytes)
                                              : out.add(h, asks[i].bytes));
    }
    const size_t total = out.total();
    const cda::OutRegions::Span span = out.span();
    std::vector<uint8_t> scratch(total + 1);
    for (size_t i = 0; i < scratch.size(); i++) scratch[i] = (uint8_t)(i * 7 + 3);
    printf("L %s : %zu %zu %zu |", name, total, span.off, span.bytes);
    for (size_t i = 0; i < regs.size(); i++) {
        const cda::OutRegions::Region& r = regs[i];
        const uint8_t* d = r.dev(scratch.data());
        printf(" %zu %zu %ld", r.off, r.bytes, d ? (long)(d - scratch.data()) : -1L);
        if ((d == nullptr) != !asks[i].host) fail(name, "device pointer and host pointer disagree");
        if (!asks[i].host && r.bytes) fail(name, "a NULL host pointer has bytes");
        if (asks[i].host && r.bytes != asks[i].bytes) fail(name, "a requested region lost bytes");
        if (asks[i].in_upload < 0) {
            if (r.off % 16) fail(name, "region not at a 16-byte boundary");
            if (r.off < upload) fail(name, "region inside the upload");
        } else if (r.off + r.bytes > upload) {
            fail(name, "region placed in the upload leaves it");
        }
        if (r.off + r.bytes > total) fail(name, "region beyond total()");
        for (size_t j = 0; j < i; j++)
            if (r.bytes && regs[j].bytes && r.off < regs[j].off + regs[j].bytes && regs[j].off < r.off + r.bytes)
                fail(name, "regions overlap");
    }
    printf("\nC %s :", name);
    size_t lo = total, hi = 0;
    for (const cda::OutRegions::Region& r : out.copies()) {
        printf(" %zu %zu", r.off, r.bytes);
        if (!r.host || !r.bytes) fail(name, "an empty region is listed for copying");
        if (r.off < lo) lo = r.off;
        if (r.off + r.bytes > hi) hi = r.off + r.bytes;
    }
    printf("\n");
    if (out.copies().empty() ? (span.off || span.bytes) : (span.off != lo || span.bytes != hi - lo))
        fail(name, "span does not cover exactly the copies");
    // both forms of the copy back deliver the same bytes and touch nothing else
    std::vector<uint8_t> stage(scratch.begin() + span.off, scratch.begin() + span.off + span.bytes);
    for (const cda::OutRegions::Region& r : out.copies()) std::memcpy(r.host, stage.data() + (r.off - span.off), r.bytes);
    for (size_t i = 0; i < asks.size(); i++) {
        const size_t n = regs[i].bytes;
        if (n && std::memcmp(host[i].data(), scratch.data() + regs[i].off, n)) fail(name, "span copy differs");
        if (host[i][n] != 0xAA) fail(name, "copy wrote beyond its region");
        if (!n && host[i][0] != 0xAA) fail(name, "an empty region was written");
    }
}

}  // namespace

int main() {
    static_assert(cda::OutRegions::align(0) == 0 && cda::OutRegions::align(1) == 16 && cda::OutRegions::align(16) == 16 &&
                  cda::OutRegions::align(17) == 32);
    // five samples at k = 2 (D = 2, A = 3): coordinates, then shares, namespaces, nodes, roots, leaf hashes, aunts
    layout_line("samples", 20, {{true, 2560, -1}, {true, 145, -1}, {true, 900, -1}, {true, 450, -1}, {true, 160, -1},
                                {true, 480, -1}});
    // the same with the namespaces and the roots not requested
    layout_line("null", 20, {{true, 2560, -1}, {false, 145, -1}, {true, 900, -1}, {false, 450, -1}, {true, 160, -1},
                             {true, 480, -1}});
    // a requested output of no bytes keeps a device pointer and is not copied
    layout_line("zero", 16, {{true, 0, -1}, {true, 29, -1}, {true, 0, -1}});
    // nothing requested: only the upload
    layout_line("none", 33, {{false, 90, -1}, {false, 32, -1}});
    // no upload, no regions
    layout_line("empty", 0, {});
    // three segments and three flag bytes in a 100-byte upload; the flags come back from inside it
    layout_line("flags", 100, {{true, 270, -1}, {false, 96, -1}, {true, 29, -1}, {true, 3, 96}});
    // only the flags
    layout_line("flags_only", 100, {{false, 270, -1}, {true, 3, 96}});
    // the flags not requested
    layout_line("no_flags", 100, {{true, 90, -1}, {false, 3, 96}});
    return failures ? 1 : 0;
}
