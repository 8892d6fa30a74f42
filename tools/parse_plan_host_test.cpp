// Host test of csrc/parse_plan.h (no GPU): the share digests, the sequence table
// and its checks, the share-count rules, the unit walk with the reserved-bytes
// check, and every error text, on squares of at most 16 shares written here by
// hand.  Prints one line per case; tests/test_parse_plan.py compares them with
// values worked out by hand.
//   D name : w0 be30 | ...                                   one pair per share
//   T name : n_blobs n_padding blob_bytes compact_bytes | start n L kind | ...
//   U name : n_txs n_pfbs unit_bytes | off len share_start share_end | ...
//   N / C / E name : numbers, or the error text
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "parse_plan.h"

using namespace cda::parse;

using Share = std::vector<uint8_t>;

static Share ns_of(uint8_t fill28, uint8_t last) {
    Share s(kNs, fill28);
    s[28] = last;
    return s;
}
static const Share kTxNs = ns_of(0x00, 0x01), kPfbNs = ns_of(0x00, 0x04), kReservedNs = ns_of(0x00, 0xFF),
                   kTailNs = ns_of(0xFF, 0xFE), kParityNs = ns_of(0xFF, 0xFF);
static Share blob_ns(uint8_t i) {
    Share s(kNs, 0);
    s[19] = 1;
    s[28] = i;
    return s;
}
static void be32(Share& s, size_t at, uint32_t v) {
    for (int i = 0; i < 4; i++) s[at + i] = (uint8_t)(v >> (24 - 8 * i));
}
// namespace | info | rest, zero filled
static Share share(const Share& ns, uint8_t info) {
    Share s(kShare, 0);
    std::memcpy(s.data(), ns.data(), kNs);
    s[kNs] = info;
    return s;
}
static Share start_share(const Share& ns, uint32_t L) {
    Share s = share(ns, 1);
    be32(s, 30, L);
    return s;
}
static Share compact_start(const Share& ns, uint32_t L, uint32_t reserved, const std::vector<uint8_t>& stream) {
    Share s = start_share(ns, L);
    be32(s, 34, reserved);
    std::memcpy(s.data() + 38, stream.data(), stream.size());
    return s;
}

static std::vector<uint8_t> flat(const std::vector<Share>& sq) {
    std::vector<uint8_t> b;
    for (const Share& s : sq) b.insert(b.end(), s.begin(), s.end());
    return b;
}

static void print_table(const char* name, const std::string& bad, const Table& t) {
    if (!bad.empty()) {
        std::printf("E %s : %s\n", name, bad.c_str());
        return;
    }
    std::printf("T %s : %u %u %llu %llu", name, t.n_blobs, t.n_padding, (unsigned long long)t.blob_bytes,
                (unsigned long long)t.compact_bytes);
    for (const Sequence& s : t.seqs) std::printf(" | %u %u %u %u", s.start, s.n, s.L, s.kind);
    std::printf("\n");
}

static void table(const char* name, const std::vector<Share>& sq, std::vector<uint32_t> starts = {},
                  std::vector<uint32_t> ends = {}) {
    const std::vector<uint8_t> raw = flat(sq);
    if (starts.empty()) {
        starts = {0};
        ends = {(uint32_t)sq.size()};
    }
    // digests of the ranges' shares in range order: a range's first share has no share before it
    std::vector<Digest> all(sq.size()), d;
    digest_shares(raw.data(), kShare, sq.size(), all.data());
    for (size_t r = 0; r < starts.size(); r++)
        for (uint32_t i = starts[r]; i < ends[r]; i++) {
            d.push_back(all[i]);
            if (i == starts[r]) d.back().w0 &= ~(1u << 16);
        }
    Table t;
    print_table(name, build_table(d.data(), starts.data(), ends.data(), (uint32_t)starts.size(), &t), t);
}

static void units(const char* name, const std::vector<Share>& sq) {
    const std::vector<uint8_t> raw = flat(sq);
    std::vector<Digest> d(sq.size());
    digest_shares(raw.data(), kShare, sq.size(), d.data());
    const uint32_t zero = 0, n = (uint32_t)sq.size();
    Parsed p;
    std::string bad = build_table(d.data(), &zero, &n, 1, &p.table);
    if (bad.empty()) {
        layout_table(&p);
        std::vector<uint8_t> compact(p.table.compact_bytes);
        for (size_t q = 0; q < p.table.seqs.size(); q++) {
            const Sequence& s = p.table.seqs[q];
            if (!s.compact()) continue;
            uint64_t left = s.L, at = p.compact_off[q];
            for (uint32_t j = 0; j < s.n && left; j++) {
                const uint32_t h = j ? s.hdr_cont() : s.hdr_first();
                const uint64_t c = left < kShare - h ? left : kShare - h;
                std::memcpy(compact.data() + at, raw.data() + (size_t)(s.start + j) * kShare + h, c);
                at += c;
                left -= c;
            }
        }
        bad = walk_table(d.data(), compact.data(), &p);
    }
    if (!bad.empty()) {
        std::printf("E %s : %s\n", name, bad.c_str());
        return;
    }
    std::printf("U %s : %u %u %llu", name, p.n_txs, p.n_pfbs, (unsigned long long)p.unit_bytes);
    for (const Unit& u : p.units)
        std::printf(" | %llu %llu %u %u", (unsigned long long)u.off, (unsigned long long)u.len, u.share_start, u.share_end);
    std::printf("\n");
}

int main() {
    // 0 tx {abc, de}; 1 pfb {wxyz}; 2 reserved padding; 3 blob 1 of 1 byte; 4-5 blob 2 of 479 bytes;
    // 6 namespace padding of blob 2's namespace; 7 tail padding
    std::vector<Share> sq;
    sq.push_back(compact_start(kTxNs, 7, 38, {3, 'a', 'b', 'c', 2, 'd', 'e'}));
    sq.push_back(compact_start(kPfbNs, 5, 38, {4, 'w', 'x', 'y', 'z'}));
    sq.push_back(start_share(kReservedNs, 0));
    sq.push_back(start_share(blob_ns(1), 1));
    sq.back()[34] = 0x55;
    sq.push_back(start_share(blob_ns(2), 479));
    sq.push_back(share(blob_ns(2), 0));
    sq.back()[30] = 0x66;
    sq.push_back(start_share(blob_ns(2), 0));
    sq.push_back(start_share(kTailNs, 0));
    {
        const std::vector<uint8_t> raw = flat(sq);
        std::vector<Digest> d(sq.size());
        digest_shares(raw.data(), kShare, sq.size(), d.data());
        std::printf("D simple :");
        for (const Digest& g : d) std::printf(" %u %u |", g.w0, g.be30);
        std::printf(" %u %u\n", d[0].be34, reserved_of(d[5]));
    }
    table("simple", sq);
    units("simple", sq);
    table("ranges", sq, {3, 7}, {6, 8});
    table("range_at_continuation", sq, {2, 5}, {3, 6});
    table("range_cuts_sequence", sq, {4}, {5});
    table("none", {});

    std::printf("N sparse : %u %u %u %u %u\n", sparse_shares_needed(1), sparse_shares_needed(478),
                sparse_shares_needed(479), sparse_shares_needed(960), sparse_shares_needed(961));
    std::printf("N compact : %u %u %u %u %u\n", compact_shares_needed(1), compact_shares_needed(474),
                compact_shares_needed(475), compact_shares_needed(952), compact_shares_needed(953));
    std::printf("C stream : %u %u %u %u | %u %u %u %u\n", compact_share_of(473), compact_share_of(474),
                compact_share_of(951), compact_share_of(952), compact_offset_of(0), compact_offset_of(473),
                compact_offset_of(474), compact_offset_of(952));

    // the table's errors, each the simple square with one change
    auto with = [&](size_t i, const Share& s) {
        std::vector<Share> c = sq;
        c[i] = s;
        return c;
    };
    table("parity", with(6, start_share(kParityNs, 0)));
    table("version", with(3, share(blob_ns(1), 3)));
    table("first_continuation", with(0, share(kTxNs, 0)));
    table("namespace_differs", with(5, share(blob_ns(3), 0)));
    table("too_few", with(5, start_share(blob_ns(2), 0)));
    table("too_many", with(6, share(blob_ns(2), 0)));
    table("padding_continued", with(7, share(blob_ns(2), 0)));
    table("compact_count", with(0, start_share(kTxNs, 475)));

    // a TX sequence of two shares at shares 2-3, L = 600: a unit of 471 bytes (prefix d7 03), one of 100 whose
    // one-byte prefix is byte 511 of share 2, one of 25 at byte 134 of share 3
    auto straddle = [&](uint32_t reserved1) {
        std::vector<uint8_t> stream(600, 0xAA);
        stream[0] = 0xD7, stream[1] = 0x03, stream[473] = 100, stream[574] = 25;
        std::vector<Share> c{start_share(kReservedNs, 0), start_share(kReservedNs, 0)};
        c.push_back(compact_start(kTxNs, 600, 38, std::vector<uint8_t>(stream.begin(), stream.begin() + 474)));
        Share s = share(kTxNs, 0);
        be32(s, 30, reserved1);
        std::memcpy(s.data() + 34, stream.data() + 474, 126);
        c.push_back(s);
        return c;
    };
    units("straddle", straddle(134));
    units("reserved_bytes", straddle(34));
    units("zero_ends_the_walk", {compact_start(kTxNs, 10, 38, {2, 'a', 'b', 0, 9, 9, 9, 9, 9, 9})});
    units("malformed_prefix", {start_share(kTailNs, 0), start_share(kTailNs, 0),
                               compact_start(kPfbNs, 20, 38, std::vector<uint8_t>(20, 0xFF))});
    units("prefix_cut_by_length", {compact_start(kTxNs, 3, 38, {1, 'a', 0x80})});
    units("unit_past_length", {compact_start(kTxNs, 61, 38, {80, 'a'})});
    units("reserved_zero", {compact_start(kTxNs, 3, 0, {2, 'a', 'b'})});

    const uint32_t s0[] = {0, 8, 4}, e0[] = {4, 12, 6};
    std::printf("E ranges_ok : %s\n", ranges_check(s0, e0, 2, 16).c_str());
    std::printf("E ranges_order : %s\n", ranges_check(s0, e0, 3, 16).c_str());
    std::printf("E ranges_beyond : %s\n", ranges_check(s0, e0, 2, 10).c_str());
    std::printf("E ranges_empty : %s\n", ranges_check(e0, s0, 1, 16).c_str());
    std::printf("E ranges_null : %s\n", ranges_check(nullptr, nullptr, 1, 16).c_str());
    return 0;
}
