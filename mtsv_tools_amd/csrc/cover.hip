// cover.hip -- mtsv_coverage (include/mtsv_amd.h): per reference sequence the reads, alignments, aligned bases and covered bases
// of the long-grain folds it is given, by the kernels of k_cover.hip.  add_fold stops once on the host: after the map pass, which
// writes scratch and counters only, and before anything is marked or added -- a call that is refused there leaves the bitmap
// and the counters byte for byte as they were.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "cover.hpp"
#include "fold.hpp"

namespace mtsv {

Coverage::Coverage(int device_) : device(device_) {
    require_device(device);
    tile = tile_from_env("MTSV_COVER_TILE", kCoverTile, 64, kCoverTileMax);
    if (const char* e = getenv("MTSV_COVER_LANE_MAX")) lane_max = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), kCoverLaneMaxMax);
    trace = getenv("MTSV_TRACE") != nullptr;
    timing = getenv("MTSV_COVER_TIMING") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    try {
        ev.create();
    } catch (...) {  // (no destructor runs for an object whose constructor throws)
        (void)hipStreamDestroy(stream);
        throw;
    }
}

Coverage::~Coverage() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    if (stream) {
        (void)hipStreamSynchronize(stream);
        (void)hipStreamDestroy(stream);
    }
}

void Coverage::add_refs(const std::vector<CoverRefs::Ref>& in) {
    const CoverRefs::Ref* first = refs.first_new(in);
    if (!first) return;  // (the binner adds every chunk once per super-batch)
    if (fixed)
        throw std::runtime_error("arg: reference (tax_id " + std::to_string((uint32_t)(first->first >> 32)) + ", gi " + std::to_string((uint32_t)first->first) +
                                 ") of " + std::to_string(first->second) + " bases is new to the table, or longer than it is there, and an add_fold has been " +
                                 "accepted: the references are fixed until mtsv_coverage_reset");
    refs.merge(in);
    laid_out = false;
}

// the table, a zeroed bitmap and zeroed counters on the device (nothing has been added: the table could still change)
void Coverage::lay_out() {
    HIP_CHECK(hipStreamSynchronize(stream));
    const uint64_t n = refs.n(), words = refs.words();
    d_key.alloc(n, "the references' keys");
    d_len.alloc(n, "the references' lengths");
    d_word_off.alloc(n + 1, "the references' word offsets");
    d_bitmap.alloc(words, "the coverage bitmap");
    d_cnt.alloc(4 * n, "the references' counters");
    if (n) {
        HIP_CHECK(hipMemcpy(d_key.p, refs.key.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_len.p, refs.len.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_word_off.p, refs.word_off.data(), (n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_cnt.p, 0, 4 * n * sizeof(uint64_t)));
    }
    if (words) HIP_CHECK(hipMemset(d_bitmap.p, 0, words * sizeof(uint64_t)));
    HIP_CHECK(hipDeviceSynchronize());
    laid_out = true;
}

void Coverage::reset() {
    fixed = false;
    if (!laid_out) return;
    HIP_CHECK(hipSetDevice(device));
    laid_out = false;  // (an error below: the next add_fold lays the table out anew)
    if (refs.n()) HIP_CHECK(hipMemsetAsync(d_cnt.p, 0, 4 * refs.n() * sizeof(uint64_t), stream));
    if (refs.words()) HIP_CHECK(hipMemsetAsync(d_bitmap.p, 0, refs.words() * sizeof(uint64_t), stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    laid_out = true;
}

void Coverage::add_fold(Fold& f, const uint32_t* read_len, uint64_t n_reads, uint32_t edit_slack, float* device_ms) {
    if (f.grain != MTSV_GRAIN_LONG)
        throw std::runtime_error("arg: coverage needs a fold at MTSV_GRAIN_LONG (the records' GIs and offsets), this one's grain is " + std::to_string(f.grain));
    if (f.device != device) throw std::runtime_error("arg: the fold is on device " + std::to_string(f.device) + ", the coverage on device " + std::to_string(device));
    if (n_reads != f.n_reads) throw std::runtime_error("arg: read lengths of " + std::to_string(n_reads) + " reads for a fold of " + std::to_string(f.n_reads));
    if (n_reads >= (1ull << 32)) throw std::runtime_error("limit: a fold of " + std::to_string(n_reads) + " reads, 2^32 or more, in mtsv_coverage_add_fold");
    if (device_ms) *device_ms = 0;
    if (!f.n) {  // (no read has a record: nothing is allocated or launched; the call was not refused, so the table is fixed)
        fixed = true;
        return;
    }
    const double t0 = timing ? now_ms() : 0;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamSynchronize(f.stream));
    if (!laid_out) lay_out();
    const uint32_t N = (uint32_t)f.n, n_refs = (uint32_t)refs.n();  // (a fold holds fewer than 2^32 records; so does a table)
    const void* rec = f.d_rec[f.cur].p;
    d_off.room(stream, n_reads + 1, "the reads' first records");
    d_min.room(stream, n_reads, "the reads' smallest edits");
    d_read_len.room(stream, n_reads, "the reads' lengths");
    d_ref.room(stream, N, "the records' references");
    d_head.room(stream, N, "the runs' heads");
    d_run.room(stream, (uint64_t)N + 1, "the records' runs");
    d_list.room(stream, N, "the work list");
    d_run_hit.room(stream, N, "the runs' flags");
    d_run_ref.room(stream, N, "the runs' references");
    d_sums.room(stream, (uint64_t)scan_tiles(N) + 1, "the scan's sums");
    d_ctr.room(stream, kCoverCounters + 1, "the counters");
    uint64_t* d_n_runs = d_ctr.p + kCoverCounters;
    // ---- what counts, where, in which run: nothing of the accumulator is touched ----
    HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, (kCoverCounters + 1) * sizeof(uint64_t), stream));
    HIP_CHECK(hipMemsetAsync(d_ctr.p + kCoverCtrFirstBad, 0xff, sizeof(uint64_t), stream));
    HIP_CHECK(hipMemcpyAsync(d_read_len.p, read_len, n_reads * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipEventRecord(ev[0], stream));
    launch_pair_bounds(stream, kCollapseGrainLong, rec, N, n_reads, d_off.p);
    HIP_CHECK(hipEventRecord(ev[1], stream));
    launch_cover_min(stream, rec, N, n_reads, d_off.p, d_min.p);
    HIP_CHECK(hipEventRecord(ev[2], stream));
    launch_cover_map(stream, rec, N, n_reads, d_min.p, edit_slack, d_key.p, d_len.p, n_refs, d_ref.p, d_head.p, d_ctr.p);
    launch_scan(stream, d_head.p, N, d_sums.p, d_n_runs, d_run.p);
    HIP_CHECK(hipEventRecord(ev[3], stream));
    uint64_t ctr[kCoverCounters + 1] = {};
    HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    // ---- the refusal point ----
    if (ctr[kCoverCtrBeyond])
        throw std::runtime_error("internal: " + std::to_string(ctr[kCoverCtrBeyond]) + " records of the fold belong to reads numbered at or above its " +
                                 std::to_string(n_reads));
    if (ctr[kCoverCtrUnknown] || ctr[kCoverCtrRange]) {
        std::string first;
        if (ctr[kCoverCtrFirstBad] < N) {
            uint32_t r[6] = {};
            HIP_CHECK(hipMemcpy(r, (const uint8_t*)rec + ctr[kCoverCtrFirstBad] * sizeof r, sizeof r, hipMemcpyDeviceToHost));
            first = "; the first is record " + std::to_string(ctr[kCoverCtrFirstBad]) + " (tax_id " + std::to_string(r[2]) + ", gi " + std::to_string(r[3]) +
                    ") at offset " + std::to_string(r[4]);
        }
        throw std::runtime_error("arg: " + std::to_string(ctr[kCoverCtrUnknown]) + " records of the fold name a reference the table does not hold, " +
                                 std::to_string(ctr[kCoverCtrRange]) + " lie at or beyond the end of theirs" + first);
    }
    const uint64_t n_counted = ctr[kCoverCtrCounted], n_runs = ctr[kCoverCounters];
    if (!n_runs || n_runs > N || n_counted > N)
        throw std::runtime_error("internal: " + std::to_string(N) + " records gave " + std::to_string(n_runs) + " runs and " + std::to_string(n_counted) + " counted");
    // ---- mark and count: nothing is refused from here on, and the table must not move under what is marked ----
    fixed = true;
    HIP_CHECK(hipMemsetAsync(d_run_hit.p, 0, n_runs * sizeof(uint32_t), stream));
    HIP_CHECK(hipEventRecord(ev[4], stream));
    launch_cover_mark(stream, rec, N, d_read_len.p, d_ref.p, d_run.p, d_len.p, d_word_off.p, n_refs, lane_max, d_bitmap.p, d_cnt.p, d_run_hit.p, d_run_ref.p,
                      d_list.p, d_ctr.p);
    HIP_CHECK(hipEventRecord(ev[5], stream));
    launch_cover_wave(stream, rec, N, d_read_len.p, d_ref.p, d_len.p, d_word_off.p, n_refs, d_list.p, d_ctr.p, d_bitmap.p);
    HIP_CHECK(hipEventRecord(ev[6], stream));
    launch_cover_reads(stream, d_n_runs, N, d_run_hit.p, d_run_ref.p, n_refs, d_cnt.p);
    HIP_CHECK(hipEventRecord(ev[7], stream));
    HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    const uint64_t n_listed = ctr[kCoverCtrList];
    if (n_listed > n_counted) throw std::runtime_error("internal: " + std::to_string(n_listed) + " of " + std::to_string(n_counted) + " counted records listed");
    float ms[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 3; k++) HIP_CHECK(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    for (int k = 3; k < 6; k++) HIP_CHECK(hipEventElapsedTime(&ms[k], ev[k + 1], ev[k + 2]));
    const float all_ms = ms[0] + ms[1] + ms[2] + ms[3] + ms[4] + ms[5];
    if (device_ms) *device_ms = all_ms;
    if (trace)
        fprintf(stderr, "[cover] %llu records of %llu reads in %llu runs, %llu counted at slack %u, %llu on the work list (lane tier up to %u words), %u references: "
                        "%.3f ms\n",
                (unsigned long long)N, (unsigned long long)n_reads, (unsigned long long)n_runs, (unsigned long long)n_counted, edit_slack,
                (unsigned long long)n_listed, lane_max, n_refs, all_ms);
    // MTSV_COVER_TIMING=1: where a call spends its time (tools/cover_ab.py reads this line)
    if (timing)
        fprintf(stderr, "[cover timing] add_fold records %llu reads %llu runs %llu counted %llu listed %llu; bounds %.3f ms, min %.3f ms, map %.3f ms, mark %.3f ms, "
                        "wave %.3f ms, reads %.3f ms, call %.3f ms\n",
                (unsigned long long)N, (unsigned long long)n_reads, (unsigned long long)n_runs, (unsigned long long)n_counted, (unsigned long long)n_listed, ms[0],
                ms[1], ms[2], ms[3], ms[4], ms[5], now_ms() - t0);
}

void Coverage::rows(std::vector<mtsv_ref_coverage>& out, float* device_ms) {
    const uint64_t n = refs.n();
    if (device_ms) *device_ms = 0;
    std::vector<uint64_t> cnt(4 * n, 0);
    float ms = 0;
    const double t0 = timing ? now_ms() : 0;
    if (laid_out && n) {  // (before the first add_fold there is nothing on the device, and nothing to count)
        HIP_CHECK(hipSetDevice(device));
        HIP_CHECK(hipMemsetAsync(d_cnt.p + 3 * n, 0, n * sizeof(uint64_t), stream));
        HIP_CHECK(hipEventRecord(ev[0], stream));
        launch_cover_pop(stream, d_bitmap.p, (uint32_t)refs.words(), d_word_off.p, (uint32_t)n, tile, d_cnt.p + 3 * n);
        HIP_CHECK(hipEventRecord(ev[1], stream));
        HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt.p, 4 * n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    }
    out.resize(n);
    for (uint64_t r = 0; r < n; r++) {
        if (cnt[3 * n + r] > refs.len[r] || cnt[n + r] < cnt[r])
            throw std::runtime_error("internal: reference " + std::to_string(r) + " of " + std::to_string(refs.len[r]) + " bases counts " +
                                     std::to_string(cnt[3 * n + r]) + " covered, " + std::to_string(cnt[r]) + " reads in " + std::to_string(cnt[n + r]) + " alignments");
        out[r] = mtsv_ref_coverage{(uint32_t)(refs.key[r] >> 32), (uint32_t)refs.key[r], refs.len[r], cnt[r], cnt[n + r], cnt[2 * n + r], cnt[3 * n + r]};
    }
    if (device_ms) *device_ms = ms;
    if (timing && laid_out)
        fprintf(stderr, "[cover timing] rows references %llu words %llu tile %u; popcount %.3f ms, call %.3f ms\n", (unsigned long long)n,
                (unsigned long long)refs.words(), tile, ms, now_ms() - t0);
}

}  // namespace mtsv
