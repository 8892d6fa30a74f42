// parse_plan.h -- the host side of parsing shares back into transactions and
// blobs (parse.hip, cda_shares_parse* / cda_square_parse*): the per-share header
// digest, the sequence table built and validated from the digests, the
// share-count rules, the walk over a compact sequence's units with the
// reserved-bytes check, and every error text.  Plain C++ (no HIP headers), so a
// host compiler builds and tests it (tools/parse_plan_host_test.cpp).
//
// The rules restate go-square v1.1.0 shares.ParseShares / parseCompactShares /
// parseSparseShares and specs/src/specs/shares.md.  Per share:
// namespace = bytes [0, 29), info = byte 29 (version = info >> 1, start = info
// & 1).  A start share opens a sequence and closes the one before it, a
// continuation extends the open one; the sequence length L is the big-endian
// word at [30, 34) of the start share.
//   padding  a start share with L = 0, or one in the tail-padding or primary-
//            reserved-padding namespace: one share, skipped and counted;
//   compact  TX or PFB namespace: raw data [38, 512) of the start share, [34, 512)
//            of a continuation, the four bytes in front being the reserved bytes;
//   sparse   every other namespace, a blob: [34, 512) then [30, 512).
// Two rules are stricter than go-square's: a malformed unit prefix or a unit
// beyond L is an error (not a silent stop), and every compact share's reserved
// bytes must name the first unit that starts in it (0 if none does).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define CDA_PARSE_HD __host__ __device__
#else
#define CDA_PARSE_HD
#endif

namespace cda {
namespace parse {

constexpr uint32_t kShare = 512, kNs = 29;
constexpr uint32_t kSparseFirst = kShare - kNs - 5, kSparseCont = kShare - kNs - 1;     // 478, 482
constexpr uint32_t kCompactFirst = kSparseFirst - 4, kCompactCont = kSparseCont - 4;   // 474, 478
constexpr uint32_t kMaxUvarint = 10;

// Class bits of a share's namespace (none set: any other namespace, a blob's).
constexpr uint32_t kClsTx = 1, kClsPfb = 2, kClsPadding = 4, kClsParity = 8;

// What the table builder keeps of one share's header: 16 bytes.
//   w0     info | class bits << 8 | (namespace equals the previous share's in range order) << 16
//   be30   big-endian word at [30, 34): L of a start share, the reserved bytes of a compact continuation
//   be34   big-endian word at [34, 38): the reserved bytes of a compact start share
struct Digest {
    uint32_t w0, be30, be34, pad;
    CDA_PARSE_HD uint32_t info() const { return w0 & 0xFF; }
    CDA_PARSE_HD uint32_t cls() const { return (w0 >> 8) & 0xFF; }
    CDA_PARSE_HD bool same_ns() const { return (w0 >> 16) & 1; }
    CDA_PARSE_HD bool start() const { return w0 & 1; }
    CDA_PARSE_HD uint32_t version() const { return (w0 & 0xFF) >> 1; }
};
static_assert(sizeof(Digest) == 16, "Digest is 16 bytes");

// The class of a namespace read through get(i) = byte i (i < 29).
template <class G>
CDA_PARSE_HD inline uint32_t classify(G get) {
    bool zeros28 = true, ff28 = true;
    for (uint32_t i = 0; i < kNs - 1; i++) {
        zeros28 = zeros28 && get(i) == 0x00;
        ff28 = ff28 && get(i) == 0xFF;
    }
    const uint32_t last = get(kNs - 1);
    if (zeros28) return last == 0x01 ? kClsTx : last == 0x04 ? kClsPfb : last == 0xFF ? kClsPadding : 0;
    if (ff28) return last == 0xFE ? kClsPadding : last == 0xFF ? kClsParity : 0;
    return 0;
}

// The digest of a share read through get(i) = byte i (i < 38).
template <class G>
CDA_PARSE_HD inline Digest digest(G get, bool same_ns) {
    Digest d;
    d.w0 = get(kNs) | classify(get) << 8 | (same_ns ? 1u << 16 : 0u);
    d.be30 = get(30) << 24 | get(31) << 16 | get(32) << 8 | get(33);
    d.be34 = get(34) << 24 | get(35) << 16 | get(36) << 8 | get(37);
    d.pad = 0;
    return d;
}

// The digests of n shares in order, share i at shares + i * stride (at least its first 38 bytes).
inline void digest_shares(const uint8_t* shares, size_t stride, uint64_t n, Digest* out) {
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* p = shares + i * stride;
        const bool same = i > 0 && !std::memcmp(p, p - stride, kNs);
        out[i] = digest([p](uint32_t j) -> uint32_t { return p[j]; }, same);
    }
}

// Shares a sequence of L bytes needs (L >= 1).
constexpr uint32_t shares_needed(uint32_t L, uint32_t first, uint32_t cont) {
    return L <= first ? 1 : 1 + (L - first + cont - 1) / cont;
}
constexpr uint32_t sparse_shares_needed(uint32_t L) { return shares_needed(L, kSparseFirst, kSparseCont); }
constexpr uint32_t compact_shares_needed(uint32_t L) { return shares_needed(L, kCompactFirst, kCompactCont); }

enum Kind : uint8_t { kSparse = 0, kTx = 1, kPfb = 2 };

struct Sequence {
    uint32_t start;   // index of its start share (row-major index of the square, or of the input)
    uint32_t at;      // position of that share's digest in the digest array (range order)
    uint32_t n;       // shares
    uint32_t L;       // sequence length in bytes
    uint8_t kind, version;
    bool compact() const { return kind != kSparse; }
    uint32_t hdr_first() const { return compact() ? kShare - kCompactFirst : kShare - kSparseFirst; }   // 38 / 34
    uint32_t hdr_cont() const { return compact() ? kShare - kCompactCont : kShare - kSparseCont; }      // 34 / 30
};

struct Table {
    std::vector<Sequence> seqs;   // blobs and compact sequences in input order; padding is only counted
    uint32_t n_blobs = 0, n_padding = 0;
    uint64_t blob_bytes = 0, compact_bytes = 0;
};

// "" or the text of the first malformed range: ranges of shares [starts[r], ends[r]) of a square of
// total shares, ascending and disjoint.
inline std::string ranges_check(const uint32_t* starts, const uint32_t* ends, uint32_t n_ranges, uint64_t total) {
    if (n_ranges && (!starts || !ends)) return "null buffer";
    uint64_t prev_end = 0;
    for (uint32_t r = 0; r < n_ranges; r++) {
        const std::string at = "range " + std::to_string(r) + ": ";
        if (starts[r] >= ends[r])
            return at + "start " + std::to_string(starts[r]) + " is not below end " + std::to_string(ends[r]);
        if (ends[r] > total)
            return at + "end " + std::to_string(ends[r]) + " is beyond the " + std::to_string(total) +
                   " shares of the original square";
        if (r && starts[r] < prev_end)
            return at + "start " + std::to_string(starts[r]) + " is below the end " + std::to_string(prev_end) +
                   " of the range before it";
        prev_end = ends[r];
    }
    return "";
}

// The sequence table of the digests of n_ranges ranges, concatenated in range order; each range is an
// input of its own.  "" or the text of the first error in share order (it names the share), *out
// unspecified then.  Per share: parity namespace, share version, then its place in a sequence; a
// sequence's share count is checked when it closes (at the next start share or the range's end).
inline std::string build_table(const Digest* d, const uint32_t* starts, const uint32_t* ends, uint32_t n_ranges,
                               Table* out) {
    Table t;
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_ranges; r++) {
        bool open = false, padding = false;
        Sequence cur{};
        auto close = [&]() -> std::string {
            if (!open) return "";
            const uint32_t need = padding ? 1 : cur.compact() ? compact_shares_needed(cur.L) : sparse_shares_needed(cur.L);
            if (cur.n != need)
                return "sequence at share " + std::to_string(cur.start) + ": length " + std::to_string(cur.L) +
                       " needs " + std::to_string(need) + " shares, found " + std::to_string(cur.n);
            if (padding) {
                t.n_padding++;
            } else {
                t.seqs.push_back(cur);
                if (cur.compact()) {
                    t.compact_bytes += cur.L;
                } else {
                    t.n_blobs++;
                    t.blob_bytes += cur.L;
                }
            }
            open = false;
            return "";
        };
        for (uint32_t i = starts[r]; i < ends[r]; i++, at++) {
            const Digest& g = d[at];
            auto sh = [i]() { return "share " + std::to_string(i) + ": "; };   // only an error pays for its text
            if (g.cls() & kClsParity) return sh() + "parity-namespace share";
            if (g.version() != 0) return sh() + "unsupported share version " + std::to_string(g.version());
            if (g.start()) {
                const std::string bad = close();
                if (!bad.empty()) return bad;
                open = true;
                padding = g.be30 == 0 || (g.cls() & kClsPadding);
                cur = Sequence{i, (uint32_t)at, 1, padding ? 0 : g.be30,
                               (uint8_t)(g.cls() & kClsTx ? kTx : g.cls() & kClsPfb ? kPfb : kSparse), (uint8_t)g.version()};
            } else {
                if (!open)
                    return sh() + (n_ranges == 1 && starts[0] == 0 ? std::string("the first share of the input")
                                                                 : "the first share of range " + std::to_string(r)) +
                           " is a continuation share";
                if (!g.same_ns())
                    return sh() + "continuation share's namespace differs from that of its sequence's start share " +
                           std::to_string(cur.start);
                cur.n++;
            }
        }
        const std::string bad = close();
        if (!bad.empty()) return bad;
    }
    *out = std::move(t);
    return "";
}

// Where byte p of a compact sequence's stream lies: the share of the sequence, and the offset in it.
constexpr uint32_t compact_share_of(uint64_t p) { return p < kCompactFirst ? 0 : 1 + (uint32_t)((p - kCompactFirst) / kCompactCont); }
constexpr uint32_t compact_offset_of(uint64_t p) {
    return p < kCompactFirst ? kShare - kCompactFirst + (uint32_t)p
                             : kShare - kCompactCont + (uint32_t)((p - kCompactFirst) % kCompactCont);
}

struct Unit {
    uint64_t off;                   // of its bytes in the stream
    uint64_t len;
    uint32_t share_start, share_end;   // the shares [start, end) that hold it, length prefix included
};

// The units of compact sequence s whose stream (its first L raw bytes) is given: uvarint length, then
// that many bytes; a uvarint of 0 ends the walk.  reserved[j]: the reserved bytes of share j of the
// sequence.  "" or the first error: walk errors in stream order, then the reserved bytes in share order.
inline std::string walk_units(const Sequence& s, const uint8_t* stream, const uint32_t* reserved,
                              std::vector<Unit>* units) {
    const uint64_t L = s.L;
    std::vector<uint32_t> first_unit(s.n, 0);   // expected reserved bytes
    uint64_t p = 0;
    while (p < L) {
        const uint64_t p0 = p;
        uint64_t v = 0;
        uint32_t nb = 0;
        bool done = false;
        while (!done) {
            if (p >= L)
                return "share " + std::to_string(s.start + compact_share_of(p0)) + ": malformed unit length prefix";
            const uint8_t c = stream[p++];
            if (nb == kMaxUvarint - 1 && c > 1)
                return "share " + std::to_string(s.start + compact_share_of(p0)) + ": malformed unit length prefix";
            v |= (uint64_t)(c & 0x7F) << (7 * nb);
            nb++;
            done = c < 0x80;
        }
        if (v == 0) break;
        if (v > L - p)
            return "share " + std::to_string(s.start + compact_share_of(p0)) + ": unit of " + std::to_string(v) +
                   " bytes runs past the sequence length " + std::to_string(L);
        const uint32_t j0 = compact_share_of(p0);
        if (first_unit[j0] == 0) first_unit[j0] = compact_offset_of(p0);
        units->push_back(Unit{p, v, s.start + j0, s.start + compact_share_of(p + v - 1) + 1});
        p += v;
    }
    for (uint32_t j = 0; j < s.n; j++)
        if (reserved[j] != first_unit[j])
            return "share " + std::to_string(s.start + j) + ": reserved bytes " + std::to_string(reserved[j]) +
                   ", expected " + std::to_string(first_unit[j]);
    return "";
}

// The reserved bytes of a compact share from its digest.
inline uint32_t reserved_of(const Digest& g) { return g.start() ? g.be34 : g.be30; }

// Everything a parse call returns but the blob bytes.
struct Parsed {
    Table table;
    std::vector<uint64_t> compact_off;   // per sequence of the table: offset of its stream in the compact buffer
                                         // (compact sequences, packed in table order), or of its bytes in the
                                         // packed blob data (sparse ones)
    std::vector<Unit> units;             // the TX sequences' units, then the PFB sequences'; off in the compact buffer
    uint32_t n_txs = 0, n_pfbs = 0;
    uint64_t unit_bytes = 0;
};

// The offsets of every sequence's bytes in its packed output.
inline void layout_table(Parsed* p) {
    uint64_t blob_at = 0, compact_at = 0;
    p->compact_off.clear();
    for (const Sequence& s : p->table.seqs) {
        uint64_t& at = s.compact() ? compact_at : blob_at;
        p->compact_off.push_back(at);
        at += s.L;
    }
}

// The unit walk of every compact sequence of p->table (layout_table done) over the compact buffer.
inline std::string walk_table(const Digest* d, const uint8_t* compact, Parsed* p) {
    std::vector<uint32_t> reserved;
    p->units.clear();
    p->n_txs = p->n_pfbs = 0;
    p->unit_bytes = 0;
    for (const uint8_t kind : {kTx, kPfb})
        for (size_t q = 0; q < p->table.seqs.size(); q++) {
            const Sequence& s = p->table.seqs[q];
            if (s.kind != kind) continue;
            reserved.resize(s.n);
            for (uint32_t j = 0; j < s.n; j++) reserved[j] = reserved_of(d[(size_t)s.at + j]);
            const size_t before = p->units.size();
            const std::string bad = walk_units(s, compact + p->compact_off[q], reserved.data(), &p->units);
            if (!bad.empty()) return bad;
            for (size_t u = before; u < p->units.size(); u++) {
                p->units[u].off += p->compact_off[q];
                p->unit_bytes += p->units[u].len;
            }
            (kind == kTx ? p->n_txs : p->n_pfbs) += (uint32_t)(p->units.size() - before);
        }
    return "";
}

}  // namespace parse
}  // namespace cda
