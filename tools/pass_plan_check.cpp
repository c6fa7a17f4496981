// pass_plan_check -- the driver's three policies by themselves (csrc/pass_plan.hpp: the cut of a slice into passes, the chunk
// bounds of a resident range, the range a lane of a host run takes), with no device and no library, so that they run under
// the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/pass_plan_check.cpp -o pass_plan_check
//   ./pass_plan_check
// Properties on every case (passes partition the slice in order, a pass is all tiled or all register, the slot cap, bounds
// ascend from 0 to n within the workspace, a take within what has arrived), and the literal values the loops gave while they
// still stood inside Batch::run_slice, run_range and run_host_parts.  Prints one summary line; exit 2 when a check fails.
#include <cstdio>
#include <cstring>

#include "../mtsv_tools_amd/csrc/pass_plan.hpp"

using namespace mtsv;

#define REQUIRE(c)                                                                            \
    do {                                                                                      \
        if (!(c)) {                                                                           \
            fprintf(stderr, "check failed at line %d (case %d): %s\n", __LINE__, (int)k, #c); \
            return 2;                                                                         \
        }                                                                                     \
    } while (0)

typedef std::vector<uint32_t> Lens;
static Lens rep(uint32_t n, uint32_t len) { return Lens(n, len); }
static Lens alt(uint32_t n, uint32_t a, uint32_t b) {
    Lens l;
    for (uint32_t i = 0; i < n; i++) l.push_back(i & 1 ? b : a);
    return l;
}
struct PassCase {
    const char* name;
    Lens lens;
    bool null_off;  // the slice's host offsets are not handed over (slice_max_len <= 256)
    uint64_t pass_reads;
    uint32_t K, G;
    int verify_mode;
    bool sw_pairs;
    uint64_t hit_cap;
};
static std::vector<PassCase> pass_cases() {
    const uint64_t cap = 1ull << 20;
    std::vector<PassCase> c = {
        {"all <= 256", {100, 150, 256, 31, 200}, false, 5, 18, 2, 0, true, cap},
        {"all <= 256, passes of two", {100, 150, 256, 31, 200}, false, 2, 18, 2, 0, true, cap},
        {"all > 256", {300, 1000, 257, 5000}, false, 4, 18, 2, 0, true, cap},
        {"all > 256, edit first", {300, 1000, 257, 5000}, false, 4, 18, 2, 1, true, cap},
        {"alternating 256 / 257", alt(6, 256, 257), false, 6, 18, 1, 0, true, cap},
        {"alternating 257 / 256", alt(5, 257, 256), false, 5, 18, 1, 0, true, cap},
        {"mixed, short runs", {100, 300, 300, 100, 253, 4000}, false, 6, 18, 2, 0, true, cap},
        {"hit_cap 2^31 - 1", rep(4, 150), true, 4, 18, 2, 0, true, 0x7fffffffull},
        {"hit_cap 2^31", rep(4, 150), true, 4, 18, 2, 0, true, 0x80000000ull},
        {"hit_cap 2^31, edit first", rep(4, 150), true, 4, 18, 2, 1, true, 0x80000000ull},
        {"one read shorter than K", {10}, false, 1, 18, 2, 0, true, cap},
        {"one read of K bases", {18}, true, 1, 18, 2, 0, true, cap},
        {"600 reads of 32767 bases", rep(600, 32767), false, 600, 18, 1, 0, true, cap},
        {"one read beyond the slot cap", {9000000, 300, 9000000}, false, 3, 18, 1, 0, true, cap},
        {"pass_reads 1", {100, 300, 300, 100}, false, 1, 18, 2, 0, true, cap},
        {"null offsets, passes of three", rep(5, 200), true, 3, 18, 2, 0, true, cap},
        {"null offsets, 256 bases", rep(7, 256), true, 7, 31, 5, 0, true, cap},
    };
    for (uint32_t len : {253u, 254u})
        for (int vm : {0, 1})
            for (bool sw : {true, false}) c.push_back({"253 / 254 bases", rep(3, len), true, 3, 18, 2, vm, sw, cap});
    return c;
}
struct WantPass {
    uint32_t nr, pass_max_len, max_ns;
    uint64_t slots;
    VerifyPath path;
    uint32_t plane_words;
};
constexpr VerifyPath T = VerifyPath::kTiled, E = VerifyPath::kEditFirst, R = VerifyPath::kRounds, P = VerifyPath::kPacked;
static const std::vector<std::vector<WantPass>> kWantPasses = {
    {{5, 256, 120, 1200, P, 0}},  // all <= 256
    {{2, 256, 120, 480, P, 0}, {2, 256, 120, 480, P, 0}, {1, 256, 120, 240, P, 0}},  // all <= 256, passes of two
    {{4, 5000, 2492, 19936, T, 0}},  // all > 256
    {{4, 5000, 2492, 19936, T, 0}},  // all > 256, edit first
    {{1, 256, 239, 478, P, 0}, {1, 257, 240, 480, T, 0}, {1, 256, 239, 478, P, 0}, {1, 257, 240, 480, T, 0}, {1, 256, 239, 478, P, 0}, {1, 257, 240, 480, T, 0}},  // alternating 256 / 257
    {{1, 257, 240, 480, T, 0}, {1, 256, 239, 478, P, 0}, {1, 257, 240, 480, T, 0}, {1, 256, 239, 478, P, 0}, {1, 257, 240, 480, T, 0}},  // alternating 257 / 256
    {{1, 100, 42, 84, R, 4}, {2, 300, 142, 568, T, 0}, {2, 253, 118, 472, R, 8}, {1, 4000, 1992, 3984, T, 0}},  // mixed, short runs
    {{4, 150, 67, 536, R, 5}},  // hit_cap 2^31 - 1
    {{4, 150, 67, 536, P, 0}},  // hit_cap 2^31
    {{4, 150, 67, 536, E, 5}},  // hit_cap 2^31, edit first
    {{1, 10, 0, 0, R, 2}},  // one read shorter than K
    {{1, 18, 1, 2, R, 2}},  // one read of K bases
    {{256, 32767, 32750, 16768000, T, 0}, {256, 32767, 32750, 16768000, T, 0}, {88, 32767, 32750, 5764000, T, 0}},  // 600 reads of 32767 bases
    {{1, 9000000, 8999983, 17999966, T, 0}, {1, 300, 283, 566, T, 0}, {1, 9000000, 8999983, 17999966, T, 0}},  // one read beyond the slot cap
    {{1, 100, 42, 84, R, 4}, {1, 300, 142, 284, T, 0}, {1, 300, 142, 284, T, 0}, {1, 100, 42, 84, R, 4}},  // pass_reads 1
    {{3, 200, 92, 552, R, 7}, {2, 200, 92, 368, R, 7}},  // null offsets, passes of three
    {{7, 256, 46, 644, P, 0}},  // null offsets, 256 bases
    {{3, 253, 118, 708, R, 8}},  // 253 bases: reference order, k_sw_pairs
    {{3, 253, 118, 708, P, 0}},  // ... MTSV_SW=packed
    {{3, 253, 118, 708, E, 8}},  // ... edit first
    {{3, 253, 118, 708, E, 8}},  // ... edit first, MTSV_SW=packed
    {{3, 254, 119, 714, P, 0}},  // 254 bases: k_evaluate whatever is set
    {{3, 254, 119, 714, P, 0}},
    {{3, 254, 119, 714, P, 0}},
    {{3, 254, 119, 714, P, 0}},
};

struct ChunkCase {
    uint64_t n, lanes, ws_reads, per_lane;
};
static std::vector<ChunkCase> chunk_cases() {
    std::vector<ChunkCase> c;
    for (uint64_t lanes : {1, 3, 8})
        for (uint64_t n : {0ull, 1ull, 3 * 32768ull - 1, 3 * 32768ull, 6 * 32768ull}) c.push_back({n, lanes, 1ull << 20, 2});
    for (uint64_t lanes : {1, 3, 8}) {
        c.push_back({lanes * 100000, lanes, 100000, 2});      // the workspace exactly
        c.push_back({lanes * 100000 - 1, lanes, 100000, 2});
        c.push_back({lanes * 100000, lanes, 100000, 1});
    }
    c.push_back({590000, 3, 100000, 2});   // the short first chunks push a full one past the workspace: a seventh chunk
    c.push_back({1500000, 8, 100000, 3});  // ... and here
    c.push_back({6 * 32768, 3, 1ull << 20, 3});  // too few reads for three chunks per lane
    c.push_back({10000000, 3, 4ull << 20, 2});
    c.push_back({500000, 3, 100000, 2});   // the error: the rounding of the short chunks leaves 100001 reads for the last
    c.push_back({300001, 1, 100000, 2});
    return c;
}
struct WantChunks {
    uint64_t k;  // 0: the error
    std::vector<uint64_t> bound;
};
static const std::vector<WantChunks> kWantChunks = {
    {1, {0, 0}},  // n 0, 1 lanes, ws 1048576, 2 per lane
    {1, {0, 1}},  // n 1, 1 lanes, ws 1048576, 2 per lane
    {1, {0, 98303}},  // n 98303, 1 lanes, ws 1048576, 2 per lane
    {1, {0, 98304}},  // n 98304, 1 lanes, ws 1048576, 2 per lane
    {1, {0, 196608}},  // n 196608, 1 lanes, ws 1048576, 2 per lane
    {1, {0, 0}},  // n 0, 3 lanes, ws 1048576, 2 per lane
    {1, {0, 1}},  // n 1, 3 lanes, ws 1048576, 2 per lane
    {1, {0, 98303}},  // n 98303, 3 lanes, ws 1048576, 2 per lane
    {3, {0, 32768, 65536, 98304}},  // n 98304, 3 lanes, ws 1048576, 2 per lane
    {3, {0, 13107, 39321, 78642, 117964, 157286, 196608}},  // n 196608, 3 lanes, ws 1048576, 2 per lane
    {1, {0, 0}},  // n 0, 8 lanes, ws 1048576, 2 per lane
    {1, {0, 1}},  // n 1, 8 lanes, ws 1048576, 2 per lane
    {1, {0, 98303}},  // n 98303, 8 lanes, ws 1048576, 2 per lane
    {1, {0, 98304}},  // n 98304, 8 lanes, ws 1048576, 2 per lane
    {1, {0, 196608}},  // n 196608, 8 lanes, ws 1048576, 2 per lane
    {1, {0, 100000}},  // n 100000, 1 lanes, ws 100000, 2 per lane
    {1, {0, 99999}},  // n 99999, 1 lanes, ws 100000, 2 per lane
    {1, {0, 100000}},  // n 100000, 1 lanes, ws 100000, 1 per lane
    {3, {0, 20000, 60000, 120000, 180000, 240000, 300000}},  // n 300000, 3 lanes, ws 100000, 2 per lane
    {3, {0, 19999, 59998, 119997, 179997, 239998, 299999}},  // n 299999, 3 lanes, ws 100000, 2 per lane
    {3, {0, 100000, 200000, 300000}},  // n 300000, 3 lanes, ws 100000, 1 per lane
    {8, {0, 8000, 24000, 48000, 80000, 120000, 168000, 224000, 288000, 352000, 416000, 480000, 544000, 608000, 672000, 736000, 800000}},  // n 800000, 8 lanes, ws 100000, 2 per lane
    {8, {0, 7999, 23998, 47997, 79996, 119995, 167994, 223993, 287992, 351992, 415993, 479994, 543995, 607996, 671997, 735998, 799999}},  // n 799999, 8 lanes, ws 100000, 2 per lane
    {8, {0, 100000, 200000, 300000, 400000, 500000, 600000, 700000, 800000}},  // n 800000, 8 lanes, ws 100000, 1 per lane
    {3, {0, 32777, 98332, 196665, 294998, 393332, 491666, 590000}},  // n 590000, 3 lanes, ws 100000, 2 per lane
    {8, {0, 9146, 27438, 54877, 91462, 137193, 192071, 256095, 329265, 402435, 475606, 548777, 621948, 695119, 768290, 841461, 914632, 987803, 1060974, 1134145, 1207316, 1280487, 1353658, 1426829, 1500000}},  // n 1500000, 8 lanes, ws 100000, 3 per lane
    {3, {0, 65536, 131072, 196608}},  // n 196608, 3 lanes, ws 1048576, 3 per lane
    {3, {0, 666666, 1999999, 3999999, 5999999, 7999999, 10000000}},  // n 10000000, 3 lanes, ws 4194304, 2 per lane
    {0, {}},  // n 500000, 3 lanes, ws 100000, 2 per lane: the error
    {1, {0, 75000, 150000, 225000, 300001}},  // n 300001, 1 lanes, ws 100000, 2 per lane
};

struct TakeCase {
    uint64_t n, next_read, avail;
    bool closed;  // nothing more will come for the range: every read has arrived, or its segment is closed
    uint64_t busy;
};
constexpr uint64_t kWs = 1ull << 20, kRampFloor = 768ull << 10, kIdleTake = 64ull << 10, kLanesUsed = 3;
// below and above 2 * ws_reads; at the ramp's floor (next_read 0), where it has reached the workspace, at the tail
static std::vector<TakeCase> take_cases() {
    std::vector<TakeCase> c;
    for (uint64_t n : std::vector<uint64_t>{1500000, 2 * kWs + 1, 10000000})
        for (uint64_t next_read : {0ull, 1000000ull, 9900000ull}) {
            if (next_read >= n) continue;
            for (uint64_t avail : std::vector<uint64_t>{0, 1000, kIdleTake - 1, kIdleTake, kRampFloor - 1, kRampFloor, kWs, 2 * kWs}) {
                if (avail > n - next_read) continue;
                for (bool closed : {false, true})
                    for (uint64_t busy : {0, 1}) c.push_back({n, next_read, avail, closed, busy});
            }
        }
    return c;
}
static const std::vector<uint64_t> kWantTakes = {
    0, 0, 0, 0, 0, 0, 1000, 1000, 0, 0, 65535, 65535, 65536, 0, 65536, 65536,
    786431, 0, 786431, 786431, 786432, 0, 786432, 786432, 1048576, 1048576, 1048576, 1048576, 0, 0, 0, 0,
    0, 0, 1000, 1000, 0, 0, 65535, 65535, 65536, 0, 65536, 65536, 0, 0, 0, 0,
    0, 0, 1000, 1000, 0, 0, 65535, 65535, 65536, 0, 65536, 65536, 786431, 0, 786431, 786431,
    786432, 786432, 786432, 786432, 786432, 786432, 786432, 786432, 786432, 786432, 786432, 786432, 0, 0, 0, 0,
    0, 0, 1000, 1000, 0, 0, 65535, 65535, 65536, 0, 65536, 65536, 786431, 0, 786431, 786431,
    786432, 786432, 786432, 786432, 786432, 786432, 786432, 786432, 0, 0, 0, 0, 0, 0, 1000, 1000,
    0, 0, 65535, 65535, 65536, 0, 65536, 65536, 786431, 0, 786431, 786431, 786432, 786432, 786432, 786432,
    786432, 786432, 786432, 786432, 786432, 786432, 786432, 786432, 0, 0, 0, 0, 0, 0, 1000, 1000,
    0, 0, 65535, 65535, 65536, 0, 65536, 65536, 786431, 0, 786431, 786431, 786432, 0, 786432, 786432,
    1048576, 1048576, 1048576, 1048576, 1048576, 1048576, 1048576, 1048576, 0, 0, 0, 0, 0, 0, 1000, 1000,
    0, 0, 65535, 65535, 65536, 0, 65536, 65536,
};

static int check_passes(size_t* n_passes) {
    const std::vector<PassCase> cases = pass_cases();
    size_t k = 0;
    REQUIRE(cases.size() == kWantPasses.size());
    for (; k < cases.size(); k++) {
        const PassCase& pc = cases[k];
        std::vector<uint32_t> off(1, 0);
        uint32_t slice_max_len = 0;
        for (uint32_t l : pc.lens) {
            off.push_back(off.back() + l);
            slice_max_len = std::max(slice_max_len, l);
        }
        const uint64_t n_slice = pc.lens.size();
        REQUIRE(!pc.null_off || slice_max_len <= kMaxRegisterReadLen);
        std::vector<WantPass> got;
        uint64_t r0 = 0;
        while (r0 < n_slice) {
            const PassPlan pl = plan_pass(pc.null_off ? nullptr : off.data(), r0, pc.pass_reads, n_slice, slice_max_len, pc.K, pc.G, pc.verify_mode,
                                          pc.sw_pairs, pc.hit_cap);
            // the passes partition the slice in order: this one begins where the last ended, is not empty and stays inside
            REQUIRE(pl.nr >= 1 && pl.nr <= pc.pass_reads && r0 + pl.nr <= n_slice);
            uint32_t longest = 0;
            for (uint64_t i = r0; i < r0 + pl.nr; i++) {
                REQUIRE((pc.lens[i] > kMaxRegisterReadLen) == pl.tiled());  // all tiled or all register
                longest = std::max(longest, pc.lens[i]);
            }
            REQUIRE(pl.pass_max_len >= longest && pl.pass_max_len <= slice_max_len);
            REQUIRE(slice_max_len <= kMaxRegisterReadLen || pl.pass_max_len == longest);
            REQUIRE(pl.max_ns == (pl.pass_max_len >= pc.K ? (pl.pass_max_len - pc.K) / pc.G + 1 : 0) && pl.slots == 2ull * pl.nr * pl.max_ns);
            REQUIRE(!(pl.tiled() && pl.nr > 1) || pl.slots <= kLongPassSlots);
            REQUIRE(!pl.myers() || (pl.pass_max_len <= kMaxMyersReadLen && pl.plane_words == myers_words(pl.pass_max_len)));
            REQUIRE(pl.myers() || pl.plane_words == 0);
            REQUIRE(pl.path != VerifyPath::kRounds || pc.hit_cap < (1ull << 31));
            got.push_back({pl.nr, pl.pass_max_len, pl.max_ns, pl.slots, pl.path, pl.plane_words});
            r0 += pl.nr;
        }
        const std::vector<WantPass>& want = kWantPasses[k];
        REQUIRE(got.size() == want.size());
        for (size_t i = 0; i < got.size(); i++)
            REQUIRE(got[i].nr == want[i].nr && got[i].pass_max_len == want[i].pass_max_len && got[i].max_ns == want[i].max_ns &&
                    got[i].slots == want[i].slots && got[i].path == want[i].path && got[i].plane_words == want[i].plane_words);
        *n_passes += got.size();
    }
    return 0;
}

static int check_chunks(size_t* n_chunks) {
    const std::vector<ChunkCase> cases = chunk_cases();
    size_t k = 0;
    REQUIRE(cases.size() == kWantChunks.size());
    for (; k < cases.size(); k++) {
        const ChunkCase& cc = cases[k];
        ChunkPlan cp;
        bool thrown = false;
        try {
            cp = plan_chunks(cc.n, cc.lanes, cc.ws_reads, cc.per_lane);
        } catch (const std::runtime_error& e) {
            thrown = !strcmp(e.what(), "arg: range holds more reads than the workspace was created for");
            REQUIRE(thrown);
        }
        REQUIRE(thrown == (kWantChunks[k].k == 0));
        if (thrown) continue;
        REQUIRE(cp.bound.size() >= 2 && cp.bound.front() == 0 && cp.bound.back() == cc.n);
        for (size_t c = 0; c + 1 < cp.bound.size(); c++) REQUIRE(cp.bound[c] <= cp.bound[c + 1] && cp.bound[c + 1] - cp.bound[c] <= cc.ws_reads);
        REQUIRE(cp.k >= 1 && cp.k <= cc.lanes && cp.k <= cp.n_chunks());
        REQUIRE(cp.k == kWantChunks[k].k && cp.bound == kWantChunks[k].bound);
        *n_chunks += cp.n_chunks();
    }
    return 0;
}

static int check_takes(size_t* n_takes) {
    const std::vector<TakeCase> cases = take_cases();
    size_t k = 0;
    REQUIRE(cases.size() == kWantTakes.size());
    for (; k < cases.size(); k++) {
        const TakeCase& tc = cases[k];
        const uint64_t take = range_take(tc.n, tc.next_read, kWs, kRampFloor, kIdleTake, kLanesUsed, tc.avail, tc.closed, tc.busy);
        REQUIRE(take <= tc.avail && take <= kWs);
        REQUIRE(!(tc.avail && tc.closed) || take > 0);  // what will not grow is not waited for
        REQUIRE(take == kWantTakes[k]);
    }
    *n_takes = cases.size();
    return 0;
}

int main() {
    size_t n_passes = 0, n_chunks = 0, n_takes = 0;
    if (int rc = check_passes(&n_passes)) return rc;
    if (int rc = check_chunks(&n_chunks)) return rc;
    if (int rc = check_takes(&n_takes)) return rc;
    printf("pass_plan_check ok (%zu passes, %zu chunks, %zu takes)\n", n_passes, n_chunks, n_takes);
    return 0;
}
