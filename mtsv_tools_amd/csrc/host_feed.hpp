// host_feed.hpp -- the arithmetic of a host run's feeder (Batch::HostRun, batch_host.hip) that is host integers only: the
// parts of the input seen as one batch, how that batch is cut into copy chunks and input segments, how a chunk's offsets are
// narrowed to segment-relative u32, how large the table of those offsets must be, and what of a segment has arrived for the
// lanes to take (pass_plan.hpp: range_take).  Plain inputs, plain results; includes nothing of HIP, so that
// tools/host_feed_check.cpp runs it on the CPU under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace mtsv {

// The parts as one batch: reads numbered through them, a virtual byte offset that ascends through them.  Empty parts are
// not kept.
struct FeedView {
    struct Part {
        const uint8_t* bases;
        const uint64_t* off;  // n + 1 offsets into bases
        uint64_t n, first, virt;  // its reads; the batch's number of its first read; the virtual offset of its first base
        bool pinned;  // its bases lie in page-locked memory: they are copied from where they lie
    };
    std::vector<Part> parts;
    uint64_t n = 0, total_bases = 0;

    // true: the part was kept and has bases -- the caller may then say that they are page-locked (parts.back().pinned)
    bool add(const uint8_t* bases, const uint64_t* off, uint64_t n_part) {
        if (!n_part) return false;
        if (!off || off[n_part] < off[0]) throw std::runtime_error("arg: read_off is not ascending");
        const uint64_t nb = off[n_part] - off[0];
        if (nb && !bases) throw std::runtime_error("arg: null bases");
        parts.push_back(Part{bases, off, n_part, n, total_bases, false});
        n += n_part;
        total_bases += nb;
        return nb != 0;
    }
    size_t part_of(uint64_t r) const {  // the part read r lies in (r == n: the last part)
        size_t k = parts.size() - 1;
        while (k > 0 && parts[k].first > r) k--;
        return k;
    }
    uint64_t virt_off(uint64_t r) const {  // virtual offset of read r's first base (r == n: the end of the batch)
        if (parts.empty()) return 0;
        const Part& v = parts[part_of(r)];
        return v.virt + (v.off[r - v.first] - v.off[0]);
    }
};

// One answer of the cursor.
struct FeedStep {
    enum Kind {
        kChunk,    // copy reads [r, e): they lie in part `part` from its read part_read on, and go to segment seg at base
                   // dst_b / read dst_r of its arena
        kSegment,  // segment seg opened at read r (nothing else of the step is set).  The caller publishes it, and from
                   // seg >= 2 waits until the reads before segment seg - 1 are through the kernels: the arena's last tenant
        kLimit     // read r alone does not fit an empty segment of cap_bases bases
    };
    Kind kind = kChunk;
    uint64_t r = 0, e = 0, seg = 0;
    uint64_t dst_b = 0, dst_r = 0, nb = 0;
    size_t part = 0;
    uint64_t part_read = 0;
    uint64_t cap_bases = 0;
    uint64_t cnt() const { return e - r; }
    std::string limit_text() const { return "limit: one read holds more bases than an input segment (" + std::to_string(cap_bases) + ")"; }
};

// The feeder's walk through the batch.  A chunk is whole reads, at least one, of one part, about chunk_bytes of bases (from
// chunk_min, doubling after every chunk up to chunk_max); it is shortened to what still fits the current segment -- the
// arena seg & 1, of cap_bases[seg & 1] bases and cap_reads[seg & 1] reads --; a new segment opens only when not even one
// read fits, and the chunk is then cut again inside it.
struct FeedCursor {
    const FeedView& v;
    uint64_t cap_bases[2], cap_reads[2];
    uint64_t chunk_max, chunk_bytes;
    uint64_t r = 0, seg = 0, seg_first_base = 0, seg_first_read = 0;

    FeedCursor(const FeedView& view, uint64_t cap_b0, uint64_t cap_r0, uint64_t cap_b1, uint64_t cap_r1, uint64_t chunk_min, uint64_t chunk_max_)
        : v(view), cap_bases{cap_b0, cap_b1}, cap_reads{cap_r0, cap_r1}, chunk_max(chunk_max_), chunk_bytes(chunk_min) {}
    bool done() const { return r >= v.n; }
    bool fits(uint64_t e) const { return v.virt_off(e) - seg_first_base <= cap_bases[seg & 1] && e - seg_first_read <= cap_reads[seg & 1]; }

    FeedStep next() {  // (not when done())
        FeedStep s;
        const FeedView::Part& src = v.parts[v.part_of(r)];
        // largest e within the part with virt_off(e) - virt_off(r) <= chunk_bytes (at least one read)
        uint64_t lo = r + 1, hi = src.first + src.n;
        const uint64_t lim = v.virt_off(r) + chunk_bytes;
        if (v.virt_off(hi) > lim) {
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) / 2;
                if (v.virt_off(mid) <= lim) lo = mid;
                else hi = mid - 1;
            }
            hi = lo;
        }
        uint64_t e = hi;
        if (!fits(e)) {  // does not fit the segment any more: shorten to what fits, or open the next segment
            lo = r, hi = e;
            while (lo < hi) {
                const uint64_t mid = (lo + hi + 1) / 2;
                if (fits(mid)) lo = mid;
                else hi = mid - 1;
            }
            if (lo == r) {
                s.r = r;
                s.cap_bases = cap_bases[seg & 1];
                s.kind = r == seg_first_read ? FeedStep::kLimit : FeedStep::kSegment;
                if (s.kind == FeedStep::kSegment) {
                    seg++;
                    seg_first_base = v.virt_off(r);
                    seg_first_read = r;
                    s.seg = seg;
                }
                return s;
            }
            e = lo;
        }
        s.r = r;
        s.e = e;
        s.seg = seg;
        s.nb = v.virt_off(e) - v.virt_off(r);
        s.dst_b = v.virt_off(r) - seg_first_base;
        s.dst_r = r - seg_first_read;
        s.part = v.part_of(r);
        s.part_read = r - src.first;
        r = e;
        chunk_bytes = std::min(chunk_max, chunk_bytes * 2);
        return s;
    }
};

// The table of narrowed offsets (h_off_all): the entry of read r of segment seg lies at r + seg, so that every segment has a
// closing entry of its own beside the next segment's first, which is 0.
inline uint64_t off_index(uint64_t r, uint64_t seg) { return r + seg; }
// Entries the table needs for a batch of n reads and total_bases bases in segments of arena_bases bases / arena_reads reads.
// (a segment is closed when the next read does not fit: two neighbours together hold more than one arena)
inline uint64_t offsets_needed(uint64_t n, uint64_t total_bases, uint64_t arena_bases, uint64_t arena_reads, bool one_segment) {
    return n + 2 + (one_segment ? 0 : 2 * (total_bases / arena_bases + n / arena_reads) + 8);
}

// Entries i0 + 1 .. i1 of a chunk narrowed: poff the chunk's offsets inside its part (poff[0]: its first read), ho the chunk's
// entries in the table, dst_b the chunk's first base inside its segment.  Entry 0 is the caller's.
struct Narrowed {
    uint32_t max_len = 0;    // the longest of reads i0 .. i1 - 1 (a length of 2^32 and more reads as UINT32_MAX, not as 0)
    bool descending = false;  // an offset below the one before it
};
inline Narrowed narrow_offsets(const uint64_t* poff, uint64_t i0, uint64_t i1, uint64_t dst_b, uint32_t* ho) {
    Narrowed nw;
    for (uint64_t i = i0 + 1; i <= i1; i++) {
        if (poff[i] < poff[i - 1]) nw.descending = true;
        nw.max_len = std::max(nw.max_len, (uint32_t)std::min<uint64_t>(poff[i] - poff[i - 1], UINT32_MAX));
        ho[i] = (uint32_t)(dst_b + (poff[i] - poff[0]));
    }
    return nw;
}

// the segment `read` lies in: the last one that begins at or before it
inline size_t segment_of(const std::vector<uint64_t>& seg_begin, uint64_t read) {
    size_t sg = seg_begin.size() - 1;
    while (seg_begin[sg] > read) sg--;
    return sg;
}

// What a lane can take behind next_read: a range stays inside one segment and within the reads [0, arrived) that have been
// copied.  closed: nothing more will arrive for that segment.
struct RangeRoom {
    size_t seg = 0;
    uint64_t seg_first = 0, avail = 0;
    bool closed = false;
};
inline RangeRoom range_room(const std::vector<uint64_t>& seg_begin, uint64_t n, uint64_t next_read, uint64_t arrived) {
    RangeRoom rr;
    rr.seg = segment_of(seg_begin, next_read);
    rr.seg_first = seg_begin[rr.seg];
    const uint64_t seg_end = rr.seg + 1 < seg_begin.size() ? seg_begin[rr.seg + 1] : n;
    const uint64_t upto = std::min(arrived, seg_end);
    rr.avail = upto > next_read ? upto - next_read : 0;
    rr.closed = arrived >= seg_end;
    return rr;
}

}  // namespace mtsv
