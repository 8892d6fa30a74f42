// parse.hip -- shares back into transactions and blobs: cda_shares_parse*
// (host only) and cda_square_parse* (a resident square's Q0, on the device).
// The mirror of square.hip's share writer; the rules and every error text are
// parse_plan.h's (go-square v1.1.0 shares.ParseShares restated).
//
// The device calls are two launches of the resident squares' gather kernel
// (proof.hip gather_kernel: one wavefront per piece, aligned 8-byte windows of
// the output, v_alignbyte for the source offset, byte stores only at a piece's
// two ends, every output byte written by exactly one lane):
//   1. the headers: bytes [0, 40) of every share of the call's ranges of Q0 (EDS
//      rows are W shares apart), one 40-byte piece per share, packed; they come
//      back and the host makes the share digests, builds and checks the sequence
//      table (parse_plan.h);
//   2. the payload: one piece per source share of the sequences kept, sparse
//      and compact alike -- bytes [h, 512) of the share, cut at the sequence
//      length, to their place in the packed output (h = 34 / 30 for a blob's
//      start share / continuation, 38 / 34 for a compact sequence's).  The compact
//      streams come back for the unit walk, the blob bytes go to the caller.
// No lane reads outside the aligned words that hold its piece's bytes, so
// nothing is read behind Q0's last share.  Algorithmic bytes: 40 read and
// written per share for the headers; the payload read and written once, plus a
// 24-byte piece entry per share uploaded for either launch.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cda.h"
#include "engine.h"
#include "parse_plan.h"

namespace cda {

namespace {

using parse::Digest;
using parse::Parsed;
using parse::Sequence;

constexpr uint32_t kHeader = 40;   // bytes of a share the digest needs, rounded up to the gather's window

// The caller's outputs but blob_data from a finished parse.  ns: the namespace of sequence s at
// ns + s.at * ns_stride.
void fill_outputs(const Parsed& p, const uint8_t* ns, size_t ns_stride, const uint8_t* compact,
                  const cda_parse_out& o) {
    uint32_t b = 0;
    if (o.blob_off) o.blob_off[0] = 0;
    for (size_t q = 0; q < p.table.seqs.size(); q++) {
        const Sequence& s = p.table.seqs[q];
        if (s.compact()) continue;
        if (o.blob_start) o.blob_start[b] = s.start;
        if (o.blob_shares) o.blob_shares[b] = s.n;
        if (o.blob_namespace) std::memcpy(o.blob_namespace + (size_t)b * parse::kNs, ns + (size_t)s.at * ns_stride, parse::kNs);
        if (o.blob_share_version) o.blob_share_version[b] = s.version;
        if (o.blob_off) o.blob_off[b + 1] = p.compact_off[q] + s.L;
        b++;
    }
    uint64_t at = 0;
    if (o.unit_off) o.unit_off[0] = 0;
    for (size_t u = 0; u < p.units.size(); u++) {
        const parse::Unit& x = p.units[u];
        if (o.unit_data) std::memcpy(o.unit_data + at, compact + x.off, x.len);
        at += x.len;
        if (o.unit_off) o.unit_off[u + 1] = at;
        if (o.unit_start) o.unit_start[u] = x.share_start;
        if (o.unit_end) o.unit_end[u] = x.share_end;
    }
}

cda_parse_plan_t plan_of(const Parsed& p) {
    return cda_parse_plan_t{p.table.n_blobs, p.n_txs, p.n_pfbs, p.table.n_padding, p.table.blob_bytes, p.unit_bytes};
}

// The raw bytes of sequence s of contiguous host shares into dst (s.L bytes).
void host_gather(const uint8_t* shares, const Sequence& s, uint8_t* dst) {
    uint64_t left = s.L;
    for (uint32_t j = 0; j < s.n && left; j++) {
        const uint32_t h = j == 0 ? s.hdr_first() : s.hdr_cont();
        const uint64_t c = std::min<uint64_t>(parse::kShare - h, left);
        std::memcpy(dst, shares + (size_t)(s.start + j) * parse::kShare + h, c);
        dst += c;
        left -= c;
    }
}

}  // namespace

// The host-only calls: plan (sizes) and / or out (outputs), either may be NULL.
int shares_parse(const uint8_t* shares, uint64_t n_shares, cda_parse_plan_t* plan, const cda_parse_out* out,
                 std::string* err) {
    if (n_shares && !shares) {
        *err = "null buffer";
        return CDA_ERR_INVALID;
    }
    if (n_shares > UINT32_MAX) {
        *err = "more than 2^32 - 1 shares";
        return CDA_ERR_INVALID;
    }
    const uint32_t n = (uint32_t)n_shares, zero = 0;
    std::vector<Digest> dig(n);
    parse::digest_shares(shares, parse::kShare, n, dig.data());
    Parsed p;
    *err = parse::build_table(dig.data(), &zero, &n, n ? 1 : 0, &p.table);
    if (!err->empty()) return CDA_ERR_SQUARE;
    parse::layout_table(&p);
    std::vector<uint8_t> compact(p.table.compact_bytes);
    for (size_t q = 0; q < p.table.seqs.size(); q++)
        if (p.table.seqs[q].compact()) host_gather(shares, p.table.seqs[q], compact.data() + p.compact_off[q]);
    *err = parse::walk_table(dig.data(), compact.data(), &p);
    if (!err->empty()) return CDA_ERR_SQUARE;
    if (plan) *plan = plan_of(p);
    if (!out) return CDA_OK;
    fill_outputs(p, shares, parse::kShare, compact.data(), *out);
    if (out->blob_data)
        for (size_t q = 0; q < p.table.seqs.size(); q++)
            if (!p.table.seqs[q].compact()) host_gather(shares, p.table.seqs[q], out->blob_data + p.compact_off[q]);
    return CDA_OK;
}

int Engine::square_parse(ResidentSquare* sq, const uint32_t* starts, const uint32_t* ends, uint32_t n_ranges,
                         cda_parse_plan_t* plan, const cda_parse_out* out) {
    const uint32_t k = sq->k, total = k * k;
    const uint32_t whole_start = 0, whole_end = total;
    if (n_ranges == 0) {   // the whole original square
        starts = &whole_start;
        ends = &whole_end;
        n_ranges = 1;
    }
    const std::string bad_range = parse::ranges_check(starts, ends, n_ranges, total);
    if (!bad_range.empty()) return fail(CDA_ERR_INVALID, bad_range);
    // fn(share, j) for the Q0 shares [first, first + count) (row-major in the k x k original square) of the EDS
    // of width 2k, whose rows are 2k shares apart
    const uint8_t* eds = sq->eds.as<uint8_t>();
    auto for_shares = [&](uint32_t first, uint32_t count, auto&& fn) {
        uint32_t col = first % k;
        const uint8_t* at = eds + ((uint64_t)(first / k) * 2 * k + col) * parse::kShare;
        for (uint32_t j = 0; j < count; j++) {
            fn(at, j);
            at += parse::kShare;
            if (++col == k) {
                col = 0;
                at += (uint64_t)k * parse::kShare;
            }
        }
    };
    hipStream_t s = stream_;

    // 1. the headers of the ranges' shares, in range order
    size_t n = 0;
    for (uint32_t r = 0; r < n_ranges; r++) n += ends[r] - starts[r];
    std::vector<GatherPiece> pieces;
    pieces.reserve(n);
    for (uint32_t r = 0; r < n_ranges; r++)
        for_shares(starts[r], ends[r] - starts[r], [&](const uint8_t* sh, uint32_t) {
            pieces.push_back(GatherPiece{sh, (uint64_t)pieces.size() * kHeader, kHeader});
        });
    std::vector<uint8_t> hdr(n * kHeader);
    CDA_TRY(square_gather_device(sq, pieces, hdr.size(), false));
    CDA_TRY(d2h(hdr.data(), sq->scratch.ptr, hdr.size(), s, "D2H parse headers"));
    CDA_TRY(sync(s));
    std::vector<Digest> dig(n);
    size_t at = 0;
    for (uint32_t r = 0; r < n_ranges; r++) {   // a range's first share has no share before it
        parse::digest_shares(hdr.data() + at * kHeader, kHeader, ends[r] - starts[r], dig.data() + at);
        at += ends[r] - starts[r];
    }
    Parsed p;
    std::string bad = parse::build_table(dig.data(), starts, ends, n_ranges, &p.table);
    if (!bad.empty()) return fail(CDA_ERR_SQUARE, bad);
    parse::layout_table(&p);

    // 2. the payload: the compact streams packed at 0, the blob bytes behind them
    const bool want_blobs = out && out->blob_data;
    const size_t blob_at = (p.table.compact_bytes + 15) & ~(size_t)15;
    pieces.clear();
    for (size_t q = 0; q < p.table.seqs.size(); q++) {
        const Sequence& x = p.table.seqs[q];
        if (!x.compact() && !want_blobs) continue;
        uint64_t dst = p.compact_off[q] + (x.compact() ? 0 : blob_at), left = x.L;
        for_shares(x.start, x.n, [&](const uint8_t* sh, uint32_t j) {
            const uint32_t h = j ? x.hdr_cont() : x.hdr_first();
            const uint32_t c = (uint32_t)std::min<uint64_t>(parse::kShare - h, left);
            if (c) pieces.push_back(GatherPiece{sh + h, dst, c});
            dst += c;
            left -= c;
        });
    }
    const size_t out_len = blob_at + (want_blobs ? p.table.blob_bytes : 0);
    CDA_TRY(square_gather_device(sq, pieces, out_len, false));
    std::vector<uint8_t> compact(p.table.compact_bytes);
    if (!compact.empty()) CDA_TRY(d2h(compact.data(), sq->scratch.ptr, compact.size(), s, "D2H parse compact"));
    CDA_TRY(sync(s));   // the pieces have left their pageable vector, the compact streams are here
    bad = parse::walk_table(dig.data(), compact.data(), &p);
    if (!bad.empty()) return fail(CDA_ERR_SQUARE, bad);
    if (plan) *plan = plan_of(p);
    if (!out) return CDA_OK;
    fill_outputs(p, hdr.data(), kHeader, compact.data(), *out);
    if (!want_blobs || p.table.blob_bytes == 0) return CDA_OK;
    CDA_TRY(d2h(out->blob_data, sq->scratch.as<uint8_t>() + blob_at, p.table.blob_bytes, s, "D2H parse blobs"));
    return sync(s);
}

}  // namespace cda
