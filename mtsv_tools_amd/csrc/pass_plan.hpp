// pass_plan.hpp -- the three policies of the driver that are arithmetic on host integers: how a slice is cut into passes
// (Batch::run_slice), how a resident range is cut into the lanes' chunks (Batch::run_range), and how many reads a lane of a
// host run takes next (Batch::HostRun::take_range; what has arrived for it: host_feed.hpp).  Plain inputs, plain results;
// includes nothing of HIP, so that tools/pass_plan_check.cpp runs them on the CPU under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace mtsv {

constexpr uint32_t kMaxRegisterReadLen = 256;  // 16 lanes x 16 read rows per lane: k_evaluate with the whole matrix band in registers
constexpr uint32_t kMaxReadLen = 32767;        // the tiled kernel's packed 16-bit cells (edit distance <= read length)
constexpr uint32_t kMaxMyersReadLen = 253;     // k_sw_pairs / k_edit_myers: the byte-wide SW score stays below 254
constexpr uint64_t kLongPassSlots = 16ull << 20;  // seed slots of one long-read pass, at most
constexpr uint64_t kLaneMinReads = 32768;      // a lane below this many reads does not fill the device

// 32-bit words per column k_edit_myers<W> runs a pass whose longest read has max_len bases with (reads up to 253 bases)
inline uint32_t myers_words(uint32_t max_len) { return std::min(std::max((max_len + 31) / 32, 2u), 8u); }

// The verify path of a pass, decided once: the tiled kernel for long reads; k_edit_myers in edit-first order; the reference
// order in rounds, k_sw_pairs + k_edit_myers (bit 31 of a work item is a flag, so hit_cap < 2^31); k_evaluate, packed, for
// what is left (reads of 254..256 bases, MTSV_SW=packed, a workspace of 2^31 seed hits or more).
enum class VerifyPath { kTiled, kEditFirst, kRounds, kPacked };

struct PassPlan {
    uint32_t nr = 0;            // reads of the pass: [r0, r0 + nr) of the slice
    uint32_t pass_max_len = 0;  // the longest of them (of the slice, when the slice has no long reads)
    uint32_t max_ns = 0;        // seed slots per strand
    uint64_t slots = 0;         // 2 * nr * max_ns
    VerifyPath path = VerifyPath::kPacked;
    uint32_t plane_words = 0;   // myers_words(pass_max_len) on the two k_edit_myers paths, else 0
    bool tiled() const { return path == VerifyPath::kTiled; }
    bool myers() const { return path == VerifyPath::kEditFirst || path == VerifyPath::kRounds; }
};

// The pass that begins at read r0 of a slice of n_slice reads, of pass_reads reads at most.  Long reads (beyond the
// register-resident kernels) run in passes of their own, through the tiled kernel: a pass is a contiguous range of reads, so
// cutting the slice at them keeps the hits in read order, and the dense per-strand seed slots of the other passes stay sized
// for ordinary reads.  A tiled pass of more than one read stays within kLongPassSlots.
// h_off: the slice's n_slice + 1 host offsets; read only (and then required) when slice_max_len > kMaxRegisterReadLen.
inline PassPlan plan_pass(const uint32_t* h_off, uint64_t r0, uint64_t pass_reads, uint64_t n_slice, uint32_t slice_max_len, uint32_t K,
                          uint32_t G, int verify_mode, bool sw_pairs, uint64_t hit_cap) {
    PassPlan pl;
    pl.nr = (uint32_t)std::min<uint64_t>(pass_reads, n_slice - r0);
    pl.pass_max_len = slice_max_len;
    bool tiled = false;
    if (slice_max_len > kMaxRegisterReadLen) {
        auto len_of = [&](uint64_t i) { return h_off[i + 1] - h_off[i]; };
        tiled = len_of(r0) > kMaxRegisterReadLen;
        uint32_t cnt = 0, ml = 0;
        while (cnt < pl.nr && (len_of(r0 + cnt) > kMaxRegisterReadLen) == tiled) {
            const uint32_t ml2 = std::max(ml, len_of(r0 + cnt));
            if (tiled && cnt && 2ull * (cnt + 1) * (ml2 >= K ? (ml2 - K) / G + 1 : 0) > kLongPassSlots) break;
            ml = ml2;
            cnt++;
        }
        pl.nr = cnt;
        pl.pass_max_len = ml;
    }
    pl.max_ns = pl.pass_max_len >= K ? (pl.pass_max_len - K) / G + 1 : 0;
    pl.slots = (uint64_t)(pl.nr * 2) * pl.max_ns;
    if (tiled) pl.path = VerifyPath::kTiled;
    else if (verify_mode == 1 && pl.pass_max_len <= kMaxMyersReadLen) pl.path = VerifyPath::kEditFirst;
    else if (sw_pairs && pl.pass_max_len <= kMaxMyersReadLen && hit_cap < 0x80000000ull) pl.path = VerifyPath::kRounds;
    pl.plane_words = pl.myers() ? myers_words(pl.pass_max_len) : 0;
    return pl;
}

// A resident range of n reads in chunks of at most ws_reads reads, handed to `lanes` lanes from a shared counter: chunk c is
// reads [bound[c], bound[c + 1]), `k` lanes work.  The lanes must not march in step (three index lookups at once, then three
// prefilters at once overlap nothing): every lane gets per_lane chunks, and the first chunk of lane i is (i + 1) / lanes of a
// full one, so the lanes stay a fraction of a chunk apart and one lane's index lookups (gather-bound) run under another
// lane's prefilter (VALU-bound).
struct ChunkPlan {
    std::vector<uint64_t> bound;
    uint64_t k = 1;
    uint64_t n_chunks() const { return bound.size() - 1; }
};
inline ChunkPlan plan_chunks(uint64_t n, uint64_t lanes, uint64_t ws_reads, uint64_t per_lane) {
    ChunkPlan cp;
    uint64_t k = n >= lanes * kLaneMinReads ? lanes : 1;
    uint64_t n_chunks = std::max<uint64_t>(k, (n + ws_reads - 1) / ws_reads);
    if (k > 1 && n >= k * per_lane * kLaneMinReads) n_chunks = std::max(n_chunks, k * per_lane);
    // (the short first chunks make the full ones longer: more chunks until a full one fits the workspace)
    while (k > 1 && n_chunks >= 2 * k && (double)n / ((double)n_chunks - (double)(k - 1) / 2.0) > (double)ws_reads) n_chunks++;
    std::vector<uint64_t>& bound = cp.bound;
    bound.assign(n_chunks + 1, n);
    bound[0] = 0;
    if (k > 1 && n_chunks >= 2 * k) {
        // sizes: per * 1/k, per * 2/k, .., per, then equal chunks of the rest
        const double per0 = (double)n / ((double)n_chunks - (double)(k - 1) / 2.0);  // full chunk size with the short ones counted
        uint64_t at = 0;
        for (uint64_t c = 0; c < k; c++) {
            at += (uint64_t)(per0 * (double)(c + 1) / (double)k);
            bound[c + 1] = std::min(at, n);
        }
        const uint64_t rest = n - bound[k], m = n_chunks - k;
        for (uint64_t c = 0; c < m; c++) bound[k + c + 1] = bound[k] + rest * (c + 1) / m;
    } else {
        for (uint64_t c = 0; c < n_chunks; c++) bound[c + 1] = n * (c + 1) / n_chunks;
    }
    for (uint64_t c = 0; c < n_chunks; c++)
        if (bound[c + 1] - bound[c] > ws_reads) throw std::runtime_error("arg: range holds more reads than the workspace was created for");
    cp.k = std::min(k, n_chunks);
    return cp;
}

// The reads a lane of a host run takes next, of the `avail` that have arrived behind next_read in its segment (0: wait).
// The ramp: a range grows with the reads already taken and falls with the reads left, between ramp_floor and ws_reads.  Less
// than that is taken when nothing more will come for the range (every read has arrived, or the segment is closed), or when
// no lane is busy and at least idle_take reads are there: an idle device starts on that little.
inline uint64_t range_take(uint64_t n, uint64_t next_read, uint64_t ws_reads, uint64_t ramp_floor, uint64_t idle_take, uint64_t n_lanes_used,
                           uint64_t avail, bool no_more_coming, uint64_t busy_lanes) {
    uint64_t want = ws_reads;
    if (n > 2 * ws_reads) {
        const uint64_t floor_reads = std::min<uint64_t>(ws_reads, ramp_floor);
        const uint64_t up = floor_reads + next_read / n_lanes_used;
        const uint64_t down = std::max(floor_reads, (n - next_read) / (n_lanes_used + 1));
        want = std::min(ws_reads, std::min(up, down));
    }
    if (avail >= want) return want;
    if (avail && no_more_coming) return avail;
    if (busy_lanes == 0 && avail >= std::min(idle_take, want)) return avail;
    return 0;
}

}  // namespace mtsv
