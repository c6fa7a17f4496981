// fold.hip -- the accumulator of assignment records that outlives a chunk (mtsv_fold, include/mtsv_amd.h).
//
// A database cut with mtsv-chunk that does not fit the device is binned chunk by chunk: a chunk's index and workspace
// are resident, the reads run, and what has to survive the chunk is folded into this accumulator -- the collapsed
// assignment records of the run, 16 or 24 bytes each, not its hits.  The accumulator is the sorted union of everything
// folded so far with one record per key (k_fold.hip), so it is bounded by what the final results file holds.  The results
// lines, the match flags and the taxa report are all derived from it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "fold.hpp"
#include "fold_records.hpp"
#include "mgindex.hpp"

namespace mtsv {

namespace {
void sort_unique(std::vector<uint32_t>& v) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
}
}  // namespace

Fold::Fold(int device_, int grain_) : device(device_), grain(grain_) {
    if (grain != MTSV_GRAIN_TAXID && grain != MTSV_GRAIN_TAXID_GI && grain != MTSV_GRAIN_LONG) throw std::runtime_error("arg: bad assignment grain");
    require_device(device);
    tile = tile_from_env("MTSV_FOLD_TILE", kFoldTile, 2, kFoldTileMax);
    text_tile = tile_from_env("MTSV_TEXT_TILE", kTextTile, 2, kTextTileMax);
    parse_tile = tile_from_env("MTSV_PARSE_TILE", kParseTile, 64, kParseTileMax);
    lca_tile = tile_from_env("MTSV_LCA_TILE", kLcaTile, 64, kLcaTileMax);
    pair_tile = tile_from_env("MTSV_PAIR_TILE", kPairTile, 64, kPairTileMax);
    if (const char* e = getenv("MTSV_PAIR_LANE_MAX")) pair_lane_max = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), kPairLaneMaxMax);
    abund_tile = tile_from_env("MTSV_ABUND_TILE", kAbundTile, 64, kAbundTileMax);
    if (const char* e = getenv("MTSV_ABUND_LANE_MAX")) abund_lane_max = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), kAbundLaneMaxMax);
    if (const char* e = getenv("MTSV_ABUND_DENSE_MAX")) abund_dense_max = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), kAbundDenseMax);
    if (const char* e = getenv("MTSV_ABUND_START_MASS")) abund_start_mass = std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 1), 1ull << 32);
    trace = getenv("MTSV_TRACE") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    ev.create();
}

Fold::~Fold() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    if (stream) (void)hipStreamSynchronize(stream);
    text.reset();
    parser.reset();
    lca_state.reset();
    pair_state.reset();
    abund_state.reset();
    if (stream) (void)hipStreamDestroy(stream);
}

void Fold::reset(uint64_t n_reads_) {
    n = 0;
    n_reads = n_reads_;
    taxa.clear();
}

void Fold::in_room(uint64_t n_b) { d_in.room(stream, n_b * rec_bytes(), "the incoming records", (1ull << 16) * rec_bytes()); }

Fold::Staged Fold::stage_write(uint64_t n_records, const char* what) {
    Staged s;
    if (n_records <= cap && d_rec[0].p) {
        s.dst = d_rec[cur ^ 1].p;
        return s;
    }
    const uint64_t ncap = std::min<uint64_t>(std::max<uint64_t>(std::max<uint64_t>(2 * cap, n_records), 1ull << 16), 0xffffffffull);
    try {
        for (auto& b : s.pair) b.alloc(ncap * rec_bytes(), what);
    } catch (const std::runtime_error&) {
        throw std::runtime_error(std::string("device: no memory for ") + what + " of " + std::to_string(ncap) + " records (two arrays)");
    }
    s.dst = s.pair[0].p;
    s.cap = ncap;
    return s;
}

void Fold::commit(Staged& s, uint64_t n_records) {
    if (s.cap) {
        for (int k = 0; k < 2; k++) d_rec[k].swap(s.pair[k]);
        cur = 0;
        cap = s.cap;
    } else {
        cur ^= 1;
    }
    n = n_records;
}

void Fold::fold_in(uint64_t n_b, std::vector<uint32_t>& new_taxa, float* device_ms) {
    const uint64_t rec = rec_bytes(), n_tot = n + n_b;
    if (n_tot >= (1ull << 32)) throw std::runtime_error("limit: the fold would hold " + std::to_string(n_tot) + " records before equal keys are joined, 2^32 or more");
    std::vector<uint32_t> u = taxa;
    u.insert(u.end(), new_taxa.begin(), new_taxa.end());
    sort_unique(u);
    if (u.size() >= (1ull << 30)) throw std::runtime_error("limit: taxa report of 2^30 TaxIDs or more");
    if (device_ms) *device_ms = 0;
    if (!n_b) {  // (nothing to merge: the source's TaxIDs still join the union)
        taxa.swap(u);
        return;
    }
    // ---- room; whatever fails here leaves the fold as it was ----
    Staged st = stage_write(n_tot, "an accumulator");
    if (trace && st.cap) fprintf(stderr, "[fold] accumulator grown from %llu to %llu records (two arrays of %llu bytes)\n", (unsigned long long)cap, (unsigned long long)st.cap, (unsigned long long)(st.cap * rec));
    const uint32_t tiles = fold_tiles(n_tot, tile);
    d_tile_cnt.room(stream, tiles, "the tiles' survivors");
    d_tile_off.room(stream, (uint64_t)tiles + 1, "the tiles' offsets");
    d_tile_sums.room(stream, (uint64_t)scan_tiles(tiles) + 2, "the scan's sums");
    sums_cap = d_tile_sums.cap - 1;  // (the total lies behind the sums)
    // ---- the fold: count, scan, write into the staged array (a new pair is read from the old one: no copy) ----
    uint64_t total = 0;
    HIP_CHECK(hipEventRecord(ev[0], stream));
    launch_fold_count(stream, grain, d_rec[cur].p, (uint32_t)n, d_in.p, (uint32_t)n_b, tile, d_tile_cnt.p);
    launch_scan(stream, d_tile_cnt.p, tiles, d_tile_sums.p, d_tile_sums.p + sums_cap, d_tile_off.p);
    launch_fold_write(stream, grain, d_rec[cur].p, (uint32_t)n, d_in.p, (uint32_t)n_b, tile, d_tile_off.p, st.dst);
    HIP_CHECK(hipEventRecord(ev[1], stream));
    HIP_CHECK(hipMemcpyAsync(&total, d_tile_sums.p + sums_cap, sizeof total, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (total > n_tot || total < std::max(n, n_b))
        throw std::runtime_error("internal: the fold of " + std::to_string(n) + " and " + std::to_string(n_b) + " records counted " + std::to_string(total));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (trace)
        fprintf(stderr, "[fold] %llu + %llu records -> %llu in %u tiles of %u: %.3f ms\n", (unsigned long long)n, (unsigned long long)n_b, (unsigned long long)total,
                tiles, tile, ms);
    commit(st, total);
    taxa.swap(u);
    if (device_ms) *device_ms = ms;
}

void Fold::add_run(Batch& src, float* device_ms) {
    if (src.parent) throw std::runtime_error("internal: fold of a lane");
    if (src.di->device != device) throw std::runtime_error("arg: the workspace is on device " + std::to_string(src.di->device) + ", the fold on device " + std::to_string(device));
    if (src.assign.mode == MTSV_ASSIGN_OFF) throw std::runtime_error("arg: the assignments of the workspace are not switched on (mtsv_batch_set_assignments)");
    if (src.assign.grain != grain) throw std::runtime_error("arg: the workspace's assignment grain is " + std::to_string(src.assign.grain) + ", the fold's " + std::to_string(grain));
    if (src.last_run == Batch::kRunHostOneSegment || src.last_run == Batch::kRunHostSegments)
        throw std::runtime_error("arg: the workspace's last run was a host batch (a fold takes runs on a resident batch: mtsv_batch_upload / _take_reads / _copy_reads + mtsv_batch_run, or mtsv_batch_merge_runs)");
    if (src.last_run != Batch::kRunResident && src.last_run != Batch::kRunMerged)
        throw std::runtime_error("arg: the workspace has no completed run on a resident batch whose assignments are still in HBM");
    uint64_t n_b = 0;
    for (const auto& sg : src.segments) n_b += sg.a_count;
    if (n + n_b >= (1ull << 32)) throw std::runtime_error("limit: the fold would hold " + std::to_string(n + n_b) + " records before equal keys are joined, 2^32 or more");
    // the TaxIDs the source brings: a run's come from its index's bins; a merged collector's records come from every chunk of
    // the merge while its index is one chunk's, so theirs are read from the records themselves, below
    const bool from_records = src.last_run == Batch::kRunMerged;
    std::vector<uint32_t> t;
    if (!from_records)
        for (const Bin& b : src.ix->host.bins) t.push_back(b.tax_id);
    HIP_CHECK(hipSetDevice(device));
    const uint64_t rec = rec_bytes();
    if (n_b) {
        in_room(n_b);
        // the run's records, which lie in its lanes' arrays stretch by stretch, next to each other (the run has returned: nothing
        // of the workspace is in flight)
        uint64_t at = 0;
        for (const auto& sg : src.segments) {
            if (!sg.a_count) continue;
            HIP_CHECK(hipMemcpyAsync(d_in.p + at * rec, sg.lane->d_assign.p + sg.a_offset * rec, sg.a_count * rec, hipMemcpyDeviceToDevice, stream));
            at += sg.a_count;
        }
        if (from_records) {  // (a collector is the rare source: its gathered records come to the host once, for the word behind the 8-byte read)
            std::vector<uint8_t> h(n_b * rec);
            HIP_CHECK(hipMemcpyAsync(h.data(), d_in.p, n_b * rec, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            t.resize(n_b);
            for (uint64_t i = 0; i < n_b; i++) memcpy(&t[i], &h[i * rec + 8], 4);
        }
    }
    sort_unique(t);
    fold_in(n_b, t, device_ms);
    // (the gather has completed with the fold: the workspace may be freed)
    HIP_CHECK(hipStreamSynchronize(stream));
}

void Fold::add_records(const void* records, uint64_t n_b, float* device_ms) {
    std::vector<uint32_t> t;
    check_fold_records(grain, records, n_b, n_reads, t);  // (keys strictly ascending, reads below n_reads)
    sort_unique(t);
    if (n + n_b >= (1ull << 32)) throw std::runtime_error("limit: the fold would hold " + std::to_string(n + n_b) + " records before equal keys are joined, 2^32 or more");
    HIP_CHECK(hipSetDevice(device));
    if (n_b) {
        in_room(n_b);
        HIP_CHECK(hipMemcpyAsync(d_in.p, records, n_b * rec_bytes(), hipMemcpyHostToDevice, stream));
    }
    fold_in(n_b, t, device_ms);
    HIP_CHECK(hipStreamSynchronize(stream));  // (the caller's array has been read)
}

void Fold::download(void** a, uint64_t* n_out, bool wide) {
    if (wide != (grain != MTSV_GRAIN_TAXID))
        throw std::runtime_error(wide ? "arg: the grain of this fold is MTSV_GRAIN_TAXID: its records are mtsv_assignment (mtsv_fold_download)"
                                      : "arg: the grain of this fold is not MTSV_GRAIN_TAXID: its records are mtsv_assignment_gi (mtsv_fold_download_gi)");
    HIP_CHECK(hipSetDevice(device));
    const uint64_t rec = rec_bytes();
    uint64_t pool_cap = 0;
    uint8_t* out = (uint8_t*)pinned_hits_alloc((n * rec + 31) / 32, &pool_cap);  // (the pool counts in 32-byte hits)
    if (n) {
        const hipError_t e = hipMemcpy(out, d_rec[cur].p, n * rec, hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            pinned_hits_release(out);
            throw_hip(e, "hipMemcpy(fold records)", __FILE__, __LINE__);
        }
    }
    *a = out;
    *n_out = n;
}

void Fold::match_flags(std::vector<uint64_t>& words, uint64_t* n_reads_out, uint64_t* n_matched) {
    const uint64_t nw = std::max<uint64_t>((n_reads + 63) / 64, 1);
    words.assign(nw, 0);
    *n_reads_out = n_reads;
    *n_matched = 0;
    if (!n) return;
    HIP_CHECK(hipSetDevice(device));
    d_flags.room(stream, nw + 2, "the match flags");
    uint64_t ctr[2] = {0, 0};
    HIP_CHECK(hipMemsetAsync(d_flags.p, 0, (nw + 2) * 8, stream));
    launch_fold_flags(stream, grain, d_rec[cur].p, (uint32_t)n, n_reads, d_flags.p, d_flags.p + nw);
    HIP_CHECK(hipMemcpyAsync(words.data(), d_flags.p, nw * 8, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(ctr, d_flags.p + nw, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (ctr[1]) throw std::runtime_error("internal: " + std::to_string(ctr[1]) + " reads of the fold are numbered at or above its " + std::to_string(n_reads) + " reads");
    *n_matched = ctr[0];
}

void Fold::taxa_report(std::vector<mtsv_taxon_stats>& rows, uint64_t* total_reads, float* device_ms) {
    rows.clear();
    *total_reads = 0;
    if (device_ms) *device_ms = 0;
    if (!n) return;
    HIP_CHECK(hipSetDevice(device));
    const uint64_t n_taxa = taxa.size(), n_cnt = 4 * n_taxa + 2;
    d_taxa.room(stream, n_taxa, "the TaxIDs");
    d_counts.room(stream, n_cnt, "the taxa's counters");
    std::vector<uint64_t> c(n_cnt);
    if (n_taxa) HIP_CHECK(hipMemcpyAsync(d_taxa.p, taxa.data(), n_taxa * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemsetAsync(d_counts.p, 0, n_cnt * 8, stream));
    HIP_CHECK(hipEventRecord(ev[0], stream));
    launch_fold_report(stream, grain, d_rec[cur].p, (uint32_t)n, d_taxa.p, (uint32_t)n_taxa, d_counts.p);
    HIP_CHECK(hipEventRecord(ev[1], stream));
    HIP_CHECK(hipMemcpyAsync(c.data(), d_counts.p, n_cnt * 8, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (c[n_cnt - 1])
        throw std::runtime_error("internal: " + std::to_string(c[n_cnt - 1]) + " (read, TaxID) pairs of the fold carry a TaxID that is not in its union of " + std::to_string(n_taxa) + " TaxIDs");
    rows.clear();
    for (uint64_t k = 0; k < n_taxa; k++) {
        const uint64_t* q = &c[4 * k];
        if (q[0] | q[1] | q[2] | q[3]) rows.push_back(mtsv_taxon_stats{taxa[k], 0, q[0], q[1], q[2], q[3]});
    }
    *total_reads = c[n_cnt - 2];
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (device_ms) *device_ms = ms;
    if (trace) fprintf(stderr, "[fold] report of %llu records over %llu taxa: %.3f ms\n", (unsigned long long)n, (unsigned long long)n_taxa, ms);
}

}  // namespace mtsv
