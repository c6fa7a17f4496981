// place.hip -- mtsv_batch_place_hits (include/mtsv_amd.h): the alignments of a workspace's hits, by the kernels of k_place.hip.
// A call is three steps -- map_hits, place_mapped, and the copies to the host -- of which mtsv_pileup_add_run (pile.hip) takes
// the first two and reads placements and ops where they lie.  A call stops twice on the host: after the map pass, which writes scratch and counters only, and after the placement kernel,
// which writes the placer's own arrays only.  Of the workspace nothing is written but the codes of an uploaded batch, with the
// bytes run() writes there: hits, assignments, statistics, flags and report are what they were, and a call that is refused at
// either stop leaves the workspace as it was; nothing is handed out before the second stop.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "batch.hpp"
#include "place.hpp"

namespace mtsv {

namespace {

uint32_t pow2_at_least(uint64_t x) {
    uint32_t p = 1;
    while (p < x) p *= 2;
    return p;
}

constexpr uint32_t kPlaceRingMax = 1u << 14;  // columns MTSV_PLACE_RING may ask for
constexpr uint32_t kPlaceBlocksMax = 2048;    // eight workgroups per CU of a 256-CU device
constexpr uint64_t kPlacementBytes = sizeof(mtsv_placement);
static_assert(sizeof(mtsv_placement) == 48, "k_place writes a placement as twelve words");

std::string hit_text(const mtsv_hit& h) {
    return "(read " + std::to_string(h.read) + ", tax_id " + std::to_string(h.tax_id) + ", gi " + std::to_string(h.gi) + ", strand " + std::to_string(h.strand) +
           ", edit " + std::to_string(h.edit) + ") at offset " + std::to_string(h.offset);
}

// an array of the page-locked pool that goes back to it unless it is handed out
struct PoolArray {
    void* p = nullptr;
    explicit PoolArray(uint64_t bytes) {
        uint64_t cap = 0;
        p = pinned_hits_alloc((bytes + 31) / 32, &cap);
    }
    ~PoolArray() {
        if (p) pinned_hits_release(p);
    }
    void* hand_out() {
        void* q = p;
        p = nullptr;
        return q;
    }
};

}  // namespace

Placer::Placer(int device_) : device(device_) {
    if (const char* e = getenv("MTSV_PLACE_RING")) ring_env = pow2_at_least(std::min<uint64_t>(strtoull(e, nullptr, 10), kPlaceRingMax));
    trace = getenv("MTSV_TRACE") != nullptr;
    timing = getenv("MTSV_PLACE_TIMING") != nullptr;
}

// the index's bins by key = tax_id << 32 | gi.  Checked on the host, before anything is made on the device: two bins of one
// (tax_id, gi) leave no way to tell which of them a hit lies in.
void Placer::build_table(Batch& b) {
    const std::vector<Bin>& bins = b.ix->host.bins;
    std::vector<std::pair<uint64_t, uint32_t>> t(bins.size());
    for (size_t k = 0; k < bins.size(); k++) t[k] = {(uint64_t)bins[k].tax_id << 32 | bins[k].gi, (uint32_t)k};
    std::sort(t.begin(), t.end());
    for (size_t k = 1; k < t.size(); k++)
        if (t[k].first == t[k - 1].first)
            throw std::runtime_error("arg: the index holds (tax_id " + std::to_string((uint32_t)(t[k].first >> 32)) + ", gi " + std::to_string((uint32_t)t[k].first) +
                                     ") in two bins, " + std::to_string(t[k - 1].second) + " and " + std::to_string(t[k].second) +
                                     ": a hit does not say which of them it lies in");
    std::vector<uint64_t> key(t.size());
    std::vector<uint32_t> bin(t.size());
    for (size_t k = 0; k < t.size(); k++) {
        key[k] = t[k].first;
        bin[k] = t[k].second;
    }
    d_key.alloc(key.size(), "the bins' keys");
    d_bin_of_key.alloc(bin.size(), "the keys' bins");
    if (!key.empty()) {
        HIP_CHECK(hipMemcpy(d_key.p, key.data(), key.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_bin_of_key.p, bin.data(), bin.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    n_keys = (uint32_t)key.size();
    table_ready = true;
}

mtsv_hit Placer::hit_at(uint64_t k) const {
    mtsv_hit h{};
    HIP_CHECK(hipMemcpy(&h, d_in.p + k, sizeof h, hipMemcpyDeviceToHost));
    return h;
}

// The first half of a placement, up to the first refusal point: the hits next to each other in d_in, each with its bin, its
// read and its op slots.  Nothing is placed yet.
void Placer::map_hits(Batch& b, const mtsv_hit* hits, uint64_t n_hits, Placed& r) {
    r = Placed{};
    const bool own = hits == nullptr;  // the hits of the workspace's last run, where they lie
    r.own = own;
    if (!b.resident)
        throw std::runtime_error(b.last_run == Batch::kRunHostOneSegment || b.last_run == Batch::kRunHostSegments
                                     ? "arg: the workspace's last run was a host batch (hits are placed against a resident batch: mtsv_batch_upload / _take_reads / "
                                       "_copy_reads)"
                                     : "arg: the workspace holds no resident batch (mtsv_batch_upload, mtsv_batch_take_reads, mtsv_batch_copy_reads)");
    if (own && b.last_run != Batch::kRunResident && b.last_run != Batch::kRunMerged)
        throw std::runtime_error("arg: the workspace has no completed run on its resident batch whose hits are still in HBM (mtsv_batch_run, mtsv_batch_merge_runs)");
    if (b.max_len > kMaxRegisterReadLen)
        throw std::runtime_error("limit: the resident batch holds a read of " + std::to_string(b.max_len) + " bases, hits are placed for reads of up to " +
                                 std::to_string(kMaxRegisterReadLen));
    uint64_t n = n_hits;
    if (own) {
        n = 0;
        for (const auto& sg : b.segments) n += sg.count;
    }
    if (n >= (1ull << 32)) throw std::runtime_error("limit: " + std::to_string(n) + " hits, 2^32 or more, in mtsv_batch_place_hits");
    HIP_CHECK(hipSetDevice(device));
    if (!table_ready) build_table(b);
    if (!n) return;  // nothing is launched
    hipStream_t s = b.stream;
    if (!ev.created()) ev.create();
    const uint32_t N = (uint32_t)n;
    d_in.room(s, n, "the hits to place");
    d_hit_bin.room(s, n, "the hits' bins");
    d_hit_read.room(s, n, "the hits' reads");
    d_cnt.room(s, n, "the hits' op slots");
    d_off.room(s, n + 1, "the hits' first op slots");
    d_sums.room(s, (uint64_t)scan_tiles(N) + 1, "the scan's sums");
    d_ctr.room(s, kPlaceCounters + 1, "the counters", 16);
    uint64_t* d_total = d_ctr.p + kPlaceCounters;
    // ---- the hits next to each other, the resident reads as codes ----
    if (own) {  // (the run has returned: nothing of the workspace is in flight)
        uint64_t at = 0;
        for (const auto& sg : b.segments) {
            if (!sg.count) continue;
            HIP_CHECK(hipMemcpyAsync(d_in.p + at, sg.lane->d_hits.p + sg.offset, sg.count * sizeof(DevHit), hipMemcpyDeviceToDevice, s));
            at += sg.count;
        }
    } else {
        HIP_CHECK(hipMemcpyAsync(d_in.p, hits, n * sizeof(DevHit), hipMemcpyHostToDevice, s));
    }
    const uint64_t nb = b.n_reads ? b.h_read_off[b.n_reads] : 0;
    // (an uploaded batch is normalised into d_codes as run() does it: the same bytes again after a run)
    if (!b.codes_resident && nb) launch_normalise(s, b.d_bases.p, b.d_codes.p, 0, nb);
    // ---- which bin, which read, how many slots: nothing is placed yet ----
    HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, (kPlaceCounters + 1) * sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(d_ctr.p + kPlaceCtrFirstBad, 0xff, sizeof(uint64_t), s));
    HIP_CHECK(hipMemsetAsync(d_ctr.p + kPlaceCtrFirstUnplaceable, 0xff, sizeof(uint64_t), s));
    HIP_CHECK(hipEventRecord(ev[0], s));
    launch_place_map(s, d_in.p, N, d_key.p, d_bin_of_key.p, n_keys, b.di->d_bins, b.d_read_off.p, (uint32_t)b.n_reads, b.mapped ? b.d_read_map.p : nullptr,
                     d_hit_bin.p, d_hit_read.p, d_cnt.p, d_ctr.p);
    launch_scan(s, d_cnt.p, N, d_sums.p, d_total, d_off.p);
    HIP_CHECK(hipEventRecord(ev[1], s));
    uint64_t ctr[kPlaceCounters + 1] = {};
    HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    // ---- the first refusal point ----
    if (ctr[kPlaceCtrUnknown] || ctr[kPlaceCtrRange] || ctr[kPlaceCtrAbsent] || ctr[kPlaceCtrStrand]) {
        std::string first;
        if (ctr[kPlaceCtrFirstBad] < n) first = "; the first is hit " + std::to_string(ctr[kPlaceCtrFirstBad]) + " " + hit_text(hit_at(ctr[kPlaceCtrFirstBad]));
        throw std::runtime_error("arg: of " + std::to_string(n) + " hits " + std::to_string(ctr[kPlaceCtrUnknown]) + " name a (tax_id, gi) the index does not hold, " +
                                 std::to_string(ctr[kPlaceCtrRange]) + " lie at or beyond the end of their bin, " + std::to_string(ctr[kPlaceCtrAbsent]) +
                                 " name a read that is not resident, " + std::to_string(ctr[kPlaceCtrStrand]) + " carry a strand above 1" + first);
    }
    const uint64_t total_ops = ctr[kPlaceCounters], span = ctr[kPlaceCtrSpan];
    if (total_ops >= (1ull << 32))
        throw std::runtime_error("limit: the hits' edit scripts may take " + std::to_string(total_ops) + " op slots, 2^32 or more, in mtsv_batch_place_hits");
    if (total_ops < n || span > 2ull * kMaxRegisterReadLen)
        throw std::runtime_error("internal: " + std::to_string(n) + " hits gave " + std::to_string(total_ops) + " op slots and a span of " + std::to_string(span));
    r.n = n;
    r.total_ops = total_ops;
    r.span = span;
}

// The second half, up to the second refusal point: the ring, the kernel, and placements and ops valid in d_out and d_ops.
void Placer::place_mapped(Batch& b, Placed& r) {
    hipStream_t s = b.stream;
    const uint64_t n = r.n, total_ops = r.total_ops, span = r.span;
    const uint32_t N = (uint32_t)n;
    uint64_t ctr[kPlaceCounters + 1] = {};
    // ---- the ring: a power of two of columns that holds every path with the column to its left ----
    const uint32_t words = myers_words(b.max_len);
    const uint32_t cols = std::max(pow2_at_least(span + 2), ring_env);
    const uint64_t lane_words = (uint64_t)cols * 2 * words;
    const uint64_t lanes_fit = std::max<uint64_t>(ring_budget / (lane_words * 4), place_threads());
    const uint32_t blocks = (uint32_t)std::min<uint64_t>({(n + place_threads() - 1) / place_threads(), lanes_fit / place_threads(), kPlaceBlocksMax});
    d_ring.room(s, lane_words * blocks * place_threads(), "the placement ring");
    d_ops.room(s, total_ops, "the edit scripts");
    d_out.room(s, n * kPlacementBytes, "the placements");
    HIP_CHECK(hipMemsetAsync(d_ops.p, 0, total_ops * sizeof(uint32_t), s));  // (the slots a hit leaves unused are handed out too)
    HIP_CHECK(hipEventRecord(ev[2], s));
    launch_place(s, words, blocks, d_in.p, N, d_hit_bin.p, d_hit_read.p, b.di->d_bins, b.di->view.n_bins, b.di->d_text, b.d_codes.p, b.d_read_off.p, d_off.p,
                 d_ring.p, cols, d_ops.p, d_out.p, d_ctr.p);
    HIP_CHECK(hipEventRecord(ev[3], s));
    HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    // ---- the second refusal point: nothing has been handed out ----
    if (ctr[kPlaceCtrBroken])
        throw std::runtime_error("internal: " + std::to_string(ctr[kPlaceCtrBroken]) + " of " + std::to_string(n) + " paths left the ring of " + std::to_string(cols) +
                                 " columns or their op slots");
    if (ctr[kPlaceCtrUnplaceable]) {
        std::string first;
        if (ctr[kPlaceCtrFirstUnplaceable] < n)
            first = "; the first is hit " + std::to_string(ctr[kPlaceCtrFirstUnplaceable]) + " " + hit_text(hit_at(ctr[kPlaceCtrFirstUnplaceable]));
        throw std::runtime_error("arg: " + std::to_string(ctr[kPlaceCtrUnplaceable]) + " of " + std::to_string(n) +
                                 " hits are unplaceable: no column of their bin's text behind the offset reaches the edit they carry" + first);
    }
    r.words = words;
    r.cols = cols;
    r.blocks = blocks;
    r.columns = ctr[kPlaceCtrColumns];
}

void Placer::place_on_device(Batch& b, const mtsv_hit* hits, uint64_t n_hits, Placed& r) {
    map_hits(b, hits, n_hits, r);
    if (!r.n) return;
    place_mapped(b, r);
    HIP_CHECK(hipEventElapsedTime(&r.ms_map, ev[0], ev[1]));
    HIP_CHECK(hipEventElapsedTime(&r.ms_place, ev[2], ev[3]));
}

void Placer::place(Batch& b, const mtsv_hit* hits, uint64_t n_hits, mtsv_placement** out, uint64_t* n_out, uint32_t** ops, uint64_t* n_ops_total,
                   float* device_ms) {
    if (device_ms) *device_ms = 0;
    const double t0 = timing ? now_ms() : 0;
    Placed r;
    map_hits(b, hits, n_hits, r);
    const uint64_t n = r.n, total_ops = r.total_ops;
    const bool own = r.own;
    PoolArray h_out(n * kPlacementBytes);
    if (!n) {  // nothing is launched
        PoolArray h_ops(0);
        *out = (mtsv_placement*)h_out.hand_out();
        *ops = (uint32_t*)h_ops.hand_out();
        *n_out = 0;
        *n_ops_total = 0;
        return;
    }
    PoolArray h_ops(total_ops * sizeof(uint32_t));
    place_mapped(b, r);
    hipStream_t s = b.stream;
    const uint32_t words = r.words, cols = r.cols, blocks = r.blocks;
    HIP_CHECK(hipMemcpyAsync(h_out.p, d_out.p, n * kPlacementBytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(h_ops.p, d_ops.p, total_ops * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipEventRecord(ev[4], s));
    HIP_CHECK(hipStreamSynchronize(s));
    float ms_map = 0, ms_place = 0, ms_down = 0;
    HIP_CHECK(hipEventElapsedTime(&ms_map, ev[0], ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms_place, ev[2], ev[3]));
    HIP_CHECK(hipEventElapsedTime(&ms_down, ev[3], ev[4]));
    if (device_ms) *device_ms = ms_map + ms_place + ms_down;
    const uint64_t ring_bytes = r.columns * 2 * words * 4;
    if (trace)
        fprintf(stderr, "[place] %llu hits (%s), %llu op slots, %u words, ring of %u columns x %u workgroups, %llu columns stored: %.3f ms\n", (unsigned long long)n,
                own ? "the last run's" : "given", (unsigned long long)total_ops, words, cols, blocks, (unsigned long long)r.columns,
                ms_map + ms_place + ms_down);
    // MTSV_PLACE_TIMING=1: where a call spends its time (tools/place_ab.py reads this line)
    if (timing)
        fprintf(stderr, "[place timing] hits %llu slots %llu words %u ring_cols %u blocks %u ring_bytes %llu; scan %.3f ms, kernel %.3f ms, download %.3f ms, "
                        "call %.3f ms\n",
                (unsigned long long)n, (unsigned long long)total_ops, words, cols, blocks, (unsigned long long)ring_bytes, ms_map, ms_place, ms_down, now_ms() - t0);
    *out = (mtsv_placement*)h_out.hand_out();
    *ops = (uint32_t*)h_ops.hand_out();
    *n_out = n;
    *n_ops_total = total_ops;
}

void Batch::place_hits(const mtsv_hit* hits, uint64_t n_hits, mtsv_placement** out, uint64_t* n_out, uint32_t** ops, uint64_t* n_ops_total, float* device_ms) {
    if (parent) throw std::runtime_error("internal: placement on a lane");
    if (!placer) placer = std::make_shared<Placer>(di->device);
    placer->place(*this, hits, n_hits, out, n_out, ops, n_ops_total, device_ms);
}

}  // namespace mtsv
