// cover.hpp -- the accumulator of coverage per reference sequence (cover.hip, k_cover.hip; mtsv_coverage, include/mtsv_amd.h).
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/mtsv_amd.h"
#include "cover_refs.hpp"
#include "dev_mem.hpp"
#include "kernels.hpp"

namespace mtsv {

struct Fold;

// Bound to a device, on a stream of its own.  The table lives on the host until the first add_fold lays it out on the device
// with the bitmap and the counters; a table that changes afterwards (only possible while no alignment has been added) is laid
// out again by the next add_fold.  The arrays of a call grow by reallocation and are kept.
struct Coverage {
    int device;
    hipStream_t stream = nullptr;
    bool trace = false, timing = false;
    uint32_t tile = kCoverTile;          // MTSV_COVER_TILE, read at creation (tests)
    uint32_t lane_max = kCoverLaneMax;   // MTSV_COVER_LANE_MAX, read at creation (tests): 0 sends every interval to the wavefront tier
    DevEvents<8> ev;
    CoverRefs refs;
    bool fixed = false;      // an add_fold has succeeded since create / reset: the table takes nothing new
    bool laid_out = false;   // the device holds this table, its bitmap and its counters
    DevBuf<uint64_t> d_key;
    DevBuf<uint32_t> d_len, d_word_off;
    DevBuf<uint64_t> d_bitmap;
    DevBuf<uint64_t> d_cnt;  // four planes of n_refs: reads, alignments, aligned bases, covered bases (filled by rows)
    // of a call
    DevBuf<uint32_t> d_off, d_min, d_read_len;           // by read
    DevBuf<uint32_t> d_ref, d_head, d_run, d_list;       // by record (run: n + 1)
    DevBuf<uint32_t> d_run_hit, d_run_ref;               // by run
    DevBuf<uint64_t> d_sums, d_ctr;                      // the scan's tile sums; kCoverCounters, then the runs

    explicit Coverage(int device);
    ~Coverage();
    Coverage(const Coverage&) = delete;
    Coverage& operator=(const Coverage&) = delete;

    // normalised references join the table; "arg: ..." for one that is new or longer once the table is fixed
    void add_refs(const std::vector<CoverRefs::Ref>& in);
    void reset();
    void add_fold(Fold& f, const uint32_t* read_len, uint64_t n_reads, uint32_t edit_slack, float* device_ms);
    void rows(std::vector<mtsv_ref_coverage>& out, float* device_ms);

   private:
    void lay_out();
};

}  // namespace mtsv

struct mtsv_coverage {
    mtsv::Coverage impl;
    explicit mtsv_coverage(int device) : impl(device) {}
};
