// host_feed_check -- the feeder's arithmetic of a host run by itself (csrc/host_feed.hpp: the parts as one batch, the cut into
// copy chunks and input segments, the narrowed offsets and the size of their table, what a lane may take), with no device and
// no library, so that it runs under the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_feed_check.cpp -o host_feed_check
//   ./host_feed_check
// Properties on every case, fixed and seeded (the chunks partition the batch in order, each inside one part and one segment
// and inside the arena, a segment opens only where no read fits, every table index below offsets_needed, a segment's entries
// begin at 0, ascend, keep their closing entry and give the virtual offsets back), and on the fixed cases the literal chunks,
// segment starts and longest reads the loop gave while it still stood inside Batch::run_host_parts.  Prints one summary
// line; exit 2 when a check fails.
#include <array>
#include <cstdio>
#include <cstring>

#include "../mtsv_tools_amd/csrc/host_feed.hpp"

using namespace mtsv;

#define REQUIRE(c)                                                                                  \
    do {                                                                                            \
        if (!(c)) {                                                                                 \
            fprintf(stderr, "check failed at line %d (case %d, %s): %s\n", __LINE__, k, name, #c);   \
            return 2;                                                                               \
        }                                                                                           \
    } while (0)

typedef std::vector<uint64_t> Offs;
static Offs offs(uint64_t start, const std::vector<uint64_t>& lens) {  // a part's n + 1 offsets
    Offs o{start};
    for (uint64_t l : lens) o.push_back(o.back() + l);
    return o;
}
static std::vector<uint64_t> rep(uint64_t n, uint64_t len) { return std::vector<uint64_t>(n, len); }
static const Offs kEmptyPart;  // a part of no reads: a null offset array

struct FeedCase {
    const char* name;
    std::vector<Offs> parts;
    uint64_t cap_bases, cap_reads, chunk_min, chunk_max;
};
enum End { kWhole, kLimit, kDescending };  // every read fed; the limit error; "not ascending" at the chunk behind the last
struct WantFeed {
    End end;
    std::vector<std::array<uint64_t, 5>> chunks;  // r, e, seg, dst_b, max_len
    std::vector<uint64_t> seg_begin;
};

static std::vector<FeedCase> feed_cases() {
    Offs descending = offs(0, rep(24, 30));
    descending[14] = descending[13] - 7;
    return {
        {"one part in one segment", {offs(0, rep(20, 30))}, 1024, 64, 64, 512},
        {"part boundary inside a segment, segment boundary inside a part", {offs(0, rep(10, 40)), offs(0, rep(25, 40))}, 600, 64, 64, 256},
        {"empty parts first, in the middle and last", {kEmptyPart, offs(0, rep(8, 25)), kEmptyPart, offs(0, rep(8, 25)), kEmptyPart}, 1024, 64, 64, 512},
        {"reads as long as the chunk bound and longer", {offs(0, {64, 10, 10, 128, 129, 200, 10, 10, 127, 1, 128, 128, 10})}, 1024, 64, 64, 128},
        {"a read of cap_bases bases", {offs(0, {10, 256, 10, 20})}, 256, 64, 64, 512},
        {"a read of cap_bases + 1 bases", {offs(0, {10, 257, 10})}, 256, 64, 64, 512},
        {"a first read of cap_bases + 1 bases", {offs(0, {257, 10})}, 256, 64, 64, 512},
        {"cap_reads binds before cap_bases", {offs(0, rep(30, 5))}, 1024, 7, 64, 512},
        {"five segments", {offs(0, rep(40, 30))}, 256, 64, 64, 512},
        {"five segments over three parts", {offs(0, rep(13, 30)), offs(5, rep(14, 30)), offs(9, rep(13, 30))}, 256, 64, 64, 128},
        {"zero-length reads at a chunk end and at a segment start", {offs(0, {64, 0, 0, 64, 64, 64, 0, 0, 50, 20, 0, 30, 0})}, 256, 5, 64, 512},
        {"zero-length reads only", {offs(0, rep(9, 0))}, 256, 4, 64, 512},
        {"no reads", {}, 256, 64, 64, 512},
        {"no reads in three parts", {kEmptyPart, kEmptyPart, kEmptyPart}, 256, 64, 64, 512},
        {"offsets that do not start at 0", {offs(1000, rep(12, 30)), offs(77, rep(12, 31))}, 512, 64, 64, 256},
        {"a descending offset inside a later chunk", {descending}, 1024, 64, 64, 512},
    };
}

// FIXED-CASE VALUES (from the loop of Batch::run_host_parts before it moved to host_feed.hpp)
static std::vector<WantFeed> feed_wants() {
    return {
        {kWhole, {{0, 2, 0, 0, 30}, {2, 6, 0, 60, 30}, {6, 14, 0, 180, 30}, {14, 20, 0, 420, 30}}, {0}},  // one part in one segment
        {kWhole, {{0, 1, 0, 0, 40}, {1, 4, 0, 40, 40}, {4, 10, 0, 160, 40}, {10, 15, 0, 400, 40}, {15, 21, 1, 0, 40}, {21, 27, 1, 240, 40}, {27, 30, 1, 480, 40}, {30, 35, 2, 0, 40}}, {0, 15, 30}},  // part boundary inside a segment, segment boundary inside a part
        {kWhole, {{0, 2, 0, 0, 25}, {2, 7, 0, 50, 25}, {7, 8, 0, 175, 25}, {8, 16, 0, 200, 25}}, {0}},  // empty parts first, in the middle and last
        {kWhole, {{0, 1, 0, 0, 64}, {1, 3, 0, 64, 10}, {3, 4, 0, 84, 128}, {4, 5, 0, 212, 129}, {5, 6, 0, 341, 200}, {6, 8, 0, 541, 10}, {8, 10, 0, 561, 127}, {10, 11, 0, 689, 128}, {11, 12, 0, 817, 128}, {12, 13, 0, 945, 10}}, {0}},  // reads as long as the chunk bound and longer
        {kWhole, {{0, 1, 0, 0, 10}, {1, 2, 1, 0, 256}, {2, 4, 2, 0, 20}}, {0, 1, 2}},  // a read of cap_bases bases
        {kLimit, {{0, 1, 0, 0, 10}}, {0, 1}},  // a read of cap_bases + 1 bases
        {kLimit, {}, {0}},  // a first read of cap_bases + 1 bases
        {kWhole, {{0, 7, 0, 0, 5}, {7, 14, 1, 0, 5}, {14, 21, 2, 0, 5}, {21, 28, 3, 0, 5}, {28, 30, 4, 0, 5}}, {0, 7, 14, 21, 28}},  // cap_reads binds before cap_bases
        {kWhole, {{0, 2, 0, 0, 30}, {2, 6, 0, 60, 30}, {6, 8, 0, 180, 30}, {8, 16, 1, 0, 30}, {16, 24, 2, 0, 30}, {24, 32, 3, 0, 30}, {32, 40, 4, 0, 30}}, {0, 8, 16, 24, 32}},  // five segments
        {kWhole, {{0, 2, 0, 0, 30}, {2, 6, 0, 60, 30}, {6, 8, 0, 180, 30}, {8, 12, 1, 0, 30}, {12, 13, 1, 120, 30}, {13, 16, 1, 150, 30}, {16, 20, 2, 0, 30}, {20, 24, 2, 120, 30}, {24, 27, 3, 0, 30}, {27, 31, 3, 90, 30}, {31, 32, 3, 210, 30}, {32, 36, 4, 0, 30}, {36, 40, 4, 120, 30}}, {0, 8, 16, 24, 32}},  // five segments over three parts
        {kWhole, {{0, 3, 0, 0, 64}, {3, 5, 0, 64, 64}, {5, 10, 1, 0, 64}, {10, 13, 2, 0, 30}}, {0, 5, 10}},  // zero-length reads at a chunk end and at a segment start
        {kWhole, {{0, 4, 0, 0, 0}, {4, 8, 1, 0, 0}, {8, 9, 2, 0, 0}}, {0, 4, 8}},  // zero-length reads only
        {kWhole, {}, {0}},  // no reads
        {kWhole, {}, {0}},  // no reads in three parts
        {kWhole, {{0, 2, 0, 0, 30}, {2, 6, 0, 60, 30}, {6, 12, 0, 180, 30}, {12, 16, 0, 360, 31}, {16, 24, 1, 0, 31}}, {0, 16}},  // offsets that do not start at 0
        {kDescending, {{0, 2, 0, 0, 30}, {2, 6, 0, 60, 30}}, {0}},  // a descending offset inside a later chunk
    };
}

// One case through the cursor as the feeder drives it: properties checked on the way, what it gave in `got`.
static int run_case(int k, const FeedCase& c, WantFeed& got) {
    const char* name = c.name;
    FeedView v;
    for (const Offs& o : c.parts) v.add((const uint8_t*)"", o.empty() ? nullptr : o.data(), o.empty() ? 0 : o.size() - 1);
    uint64_t n = 0;
    for (const Offs& o : c.parts) n += o.empty() ? 0 : o.size() - 1;
    REQUIRE(v.n == n && v.virt_off(0) == 0 && v.virt_off(n) == v.total_bases);
    for (const auto& p : v.parts) REQUIRE(p.n > 0 && v.part_of(p.first) == (size_t)(&p - v.parts.data()) && v.virt_off(p.first) == p.virt);
    const bool one_segment = v.total_bases <= c.cap_bases && n <= c.cap_reads;
    std::vector<uint32_t> table(offsets_needed(n, v.total_bases, c.cap_bases, c.cap_reads, one_segment), 0xdeadbeefu);
    std::vector<int64_t> owner(table.size(), -1);  // the segment that wrote an entry
    got = WantFeed{kWhole, {}, {0}};
    FeedCursor cur(v, c.cap_bases, c.cap_reads, c.cap_bases, c.cap_reads, c.chunk_min, c.chunk_max);
    uint64_t at = 0, chunk_bytes = c.chunk_min;
    while (!cur.done()) {
        const FeedStep s = cur.next();
        const uint64_t seg_first = got.seg_begin.back(), seg_base = v.virt_off(seg_first);
        if (s.kind == FeedStep::kLimit) {
            REQUIRE(s.r == at && at == seg_first && v.virt_off(at + 1) - v.virt_off(at) > c.cap_bases);
            REQUIRE(s.limit_text() == "limit: one read holds more bases than an input segment (" + std::to_string(c.cap_bases) + ")");
            got.end = kLimit;
            return 0;
        }
        if (s.kind == FeedStep::kSegment) {  // only where not even read `at` fits what is left of the segment
            REQUIRE(s.r == at && at > seg_first && s.seg == got.seg_begin.size());
            REQUIRE(v.virt_off(at + 1) - seg_base > c.cap_bases || at + 1 - seg_first > c.cap_reads);
            got.seg_begin.push_back(at);
            continue;
        }
        REQUIRE(s.kind == FeedStep::kChunk && s.r == at && s.e > s.r && s.e <= n && s.seg == got.seg_begin.size() - 1);
        const FeedView::Part& p = v.parts[s.part];
        REQUIRE(s.r >= p.first && s.e <= p.first + p.n && s.part_read == s.r - p.first);
        REQUIRE(s.dst_b == v.virt_off(s.r) - seg_base && s.dst_r == s.r - seg_first && s.nb == v.virt_off(s.e) - v.virt_off(s.r));
        REQUIRE(s.dst_b + s.nb <= c.cap_bases && s.dst_r + s.cnt() <= c.cap_reads);
        REQUIRE(s.cnt() == 1 || s.nb <= chunk_bytes);
        chunk_bytes = std::min(c.chunk_max, chunk_bytes * 2);
        // its offsets, as the feeder writes them: entry 0 by whoever begins the segment, the rest narrowed -- here in three
        // pieces, as the packer's threads would
        const uint64_t i0 = off_index(s.r, s.seg), cnt = s.cnt();
        REQUIRE(i0 + cnt < table.size());
        uint32_t* ho = table.data() + i0;
        if (s.dst_r == 0) {
            REQUIRE(owner[i0] == -1);  // never the closing entry of the segment before
            ho[0] = 0;
            owner[i0] = (int64_t)s.seg;
        }
        REQUIRE(owner[i0] == (int64_t)s.seg);
        const uint64_t* poff = p.off + s.part_read;
        Narrowed nw;
        for (uint64_t a = 0; a < cnt;) {
            const uint64_t b = std::min(cnt, a + (cnt + 2) / 3);
            const Narrowed piece = narrow_offsets(poff, a, b, s.dst_b, ho);
            nw.max_len = std::max(nw.max_len, piece.max_len);
            nw.descending |= piece.descending;
            a = b;
        }
        if (nw.descending) {
            got.end = kDescending;
            return 0;
        }
        for (uint64_t i = 1; i <= cnt; i++) {
            REQUIRE(owner[i0 + i] == -1);
            owner[i0 + i] = (int64_t)s.seg;
        }
        uint32_t longest = 0;
        for (uint64_t i = 0; i <= cnt; i++) {
            REQUIRE(seg_base + ho[i] == v.virt_off(s.r + i));
            if (i) REQUIRE(ho[i] >= ho[i - 1]);
            if (i) longest = std::max(longest, ho[i] - ho[i - 1]);
        }
        REQUIRE(nw.max_len == longest);
        got.chunks.push_back({s.r, s.e, s.seg, s.dst_b, nw.max_len});
        at = s.e;
    }
    REQUIRE(at == n);
    // what the lanes see: every segment's entries from 0, with a closing entry of its own
    for (size_t sg = 0; sg < got.seg_begin.size() && n; sg++) {
        const uint64_t first = got.seg_begin[sg], end = sg + 1 < got.seg_begin.size() ? got.seg_begin[sg + 1] : n;
        REQUIRE(table[off_index(first, sg)] == 0 && owner[off_index(end, sg)] == (int64_t)sg);
        REQUIRE(table[off_index(end, sg)] == v.virt_off(end) - v.virt_off(first));
        for (uint64_t r = first; r < end; r++) REQUIRE(segment_of(got.seg_begin, r) == sg);
    }
    return 0;
}

// seeded cases for the properties: a few parts, some empty, short and zero-length reads and now and then one that fills an arena
static FeedCase seeded_case(uint32_t seed) {
    uint64_t x = 0x9e3779b97f4a7c15ull * (seed + 1);
    auto rnd = [&](uint64_t m) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return x % m;
    };
    FeedCase c{"seeded", {}, 256ull << rnd(3), 4 + rnd(60), 64ull << rnd(2), 256ull << rnd(2)};
    const uint64_t n_parts = 1 + rnd(5);
    for (uint64_t p = 0; p < n_parts; p++) {
        if (rnd(4) == 0) {
            c.parts.push_back(kEmptyPart);
            continue;
        }
        std::vector<uint64_t> lens;
        for (uint64_t i = 1 + rnd(40); i > 0; i--) lens.push_back(rnd(8) == 0 ? 0 : rnd(16) == 0 ? c.cap_bases - rnd(3) : 1 + rnd(90));
        c.parts.push_back(offs(rnd(1000), lens));
    }
    return c;
}

int main() {
    const std::vector<FeedCase> cases = feed_cases();
    const std::vector<WantFeed> wants = feed_wants();
    int k = 0;
    const char* name = "";
    REQUIRE(wants.size() == cases.size());
    for (; k < (int)cases.size(); k++) {
        name = cases[k].name;
        WantFeed got;
        if (int rc = run_case(k, cases[k], got)) return rc;
        REQUIRE(got.end == wants[k].end);
        REQUIRE(got.chunks == wants[k].chunks);
        REQUIRE(got.seg_begin == wants[k].seg_begin);
    }
    int n_seeded = 0;
    for (uint32_t seed = 0; seed < 400; seed++, k++, n_seeded++) {
        const FeedCase c = seeded_case(seed);
        name = c.name;
        WantFeed got;
        if (int rc = run_case(k, c, got)) return rc;
    }
    // the view's refusals
    name = "refusals";
    {
        const uint64_t down[3] = {10, 20, 5}, up[2] = {0, 4};
        FeedView v;
        bool threw = false;
        try {
            v.add((const uint8_t*)"", down, 2);
        } catch (const std::runtime_error& e) {
            threw = !strcmp(e.what(), "arg: read_off is not ascending");
        }
        REQUIRE(threw);
        threw = false;
        try {
            v.add((const uint8_t*)"", nullptr, 2);
        } catch (const std::runtime_error& e) {
            threw = !strcmp(e.what(), "arg: read_off is not ascending");
        }
        REQUIRE(threw);
        threw = false;
        try {
            v.add(nullptr, up, 1);
        } catch (const std::runtime_error& e) {
            threw = !strcmp(e.what(), "arg: null bases");
        }
        REQUIRE(threw && v.n == 0 && v.parts.empty());
        const uint64_t flat[3] = {7, 7, 7};
        REQUIRE(!v.add(nullptr, up, 0) && v.parts.empty());  // no read: not kept, nothing looked at
        REQUIRE(!v.add(nullptr, flat, 2));  // no base: no array needed, and nothing that could be page-locked
        REQUIRE(v.n == 2 && v.total_bases == 0 && !v.parts[0].pinned);
        REQUIRE(v.add((const uint8_t*)"", up, 1));
        REQUIRE(v.n == 3 && v.total_bases == 4 && !v.parts[1].pinned && v.part_of(2) == 1 && v.part_of(3) == 1 && v.virt_off(3) == 4);
    }
    // narrowing: a read of 2^32 bases and more does not read as a short one; the entries are the offsets modulo 2^32
    name = "narrowing";
    {
        const uint64_t poff[4] = {5, 5 + (1ull << 32), 6 + (1ull << 33), 6 + (1ull << 33)};
        uint32_t ho[4] = {0, 0, 0, 0};
        const Narrowed nw = narrow_offsets(poff, 0, 3, 3, ho);
        REQUIRE(nw.max_len == UINT32_MAX && !nw.descending && ho[1] == 3 && ho[2] == 4 && ho[3] == 4);
    }
    // what a lane may take: segments {0, 10, 25} of 40 reads
    name = "range_room";
    {
        const std::vector<uint64_t> sb = {0, 10, 25};
        struct { uint64_t next_read, arrived; size_t seg; uint64_t seg_first, avail; bool closed; } want[] = {
            {0, 0, 0, 0, 0, false},   {0, 4, 0, 0, 4, false},    {3, 10, 0, 0, 7, true},    {3, 30, 0, 0, 7, true},   {10, 10, 1, 10, 0, false},
            {10, 24, 1, 10, 14, false}, {12, 25, 1, 10, 13, true}, {25, 24, 2, 25, 0, false}, {30, 39, 2, 25, 9, false}, {30, 40, 2, 25, 10, true},
        };
        for (auto& w : want) {
            const RangeRoom rr = range_room(sb, 40, w.next_read, w.arrived);
            REQUIRE(rr.seg == w.seg && rr.seg_first == w.seg_first && rr.avail == w.avail && rr.closed == w.closed);
        }
        const RangeRoom one = range_room({0}, 0, 0, 0);
        REQUIRE(one.seg == 0 && one.avail == 0 && one.closed);
    }
    // the table's size: the production sizes, one segment and several
    name = "offsets_needed";
    REQUIRE(offsets_needed(1000, 150000, 3ull << 30, 1ull << 30, true) == 1002);
    REQUIRE(offsets_needed(100000000, 15000000000ull, 3ull << 30, 1ull << 30, false) == 100000000 + 2 + 2 * 4 + 8);
    REQUIRE(off_index(17, 0) == 17 && off_index(17, 3) == 20);
    printf("host_feed_check ok: %d fixed cases, %d seeded cases\n", (int)cases.size(), n_seeded);
    return 0;
}
