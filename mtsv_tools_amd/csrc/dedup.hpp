// dedup.hpp -- the map from the reads of a batch to the first read with the same codes (dedup.hip, k_dedup.hip).
#pragma once
#include <cstdint>

#include "../../include/mtsv_amd.h"
#include "batch.hpp"
#include "fold.hpp"

namespace mtsv {

// Holds what the last take_unique found: per resident read j of its source, in HBM, the caller's number of j (read, strictly
// ascending) and of the first read identical to j (rep).  The two arrays lie in two pairs that take turns, so that a take
// that is refused leaves the map as it was.  Bound to a device; it keeps no pointer to a workspace or a fold.
struct DupMap {
    int device;
    uint32_t hash_bits = 64;      // MTSV_DEDUP_HASH_BITS, read at creation (tests)
    uint32_t fan_tile = kFanTile;  // MTSV_FAN_TILE, read at creation (tests)
    bool trace = false;
    uint32_t *d_read[2] = {nullptr, nullptr}, *d_rep[2] = {nullptr, nullptr};  // cap entries each
    uint64_t cap = 0;
    int cur = 0;
    bool valid = false;  // a take has succeeded
    uint64_t n = 0, n_unique = 0;
    // scratch of a take
    uint64_t *d_hash = nullptr, *d_table = nullptr, *d_words = nullptr, *d_ctr = nullptr;
    uint32_t* d_slot = nullptr;
    uint64_t reads_cap = 0, table_cap = 0;
    hipEvent_t ev[8] = {};
    float ms_hash = 0, ms_insert = 0, ms_resolve = 0, ms_scan = 0, ms_copy = 0;  // of the last take
    // scratch of an expansion (the map itself is not changed by one)
    struct Fan {
        uint32_t *d_first = nullptr, *d_cnt = nullptr, *d_off = nullptr;  // cap, cap, cap + 1 entries
        uint64_t* d_sums = nullptr;                                      // the scan's tile sums, then its total, then the counter
        uint64_t cap = 0, sums_cap = 0;
        hipEvent_t ev[4] = {};  // around count + scan, around write
    };
    mutable Fan fan;

    explicit DupMap(int device);
    ~DupMap();
    DupMap(const DupMap&) = delete;
    DupMap& operator=(const DupMap&) = delete;

    // dst's resident batch := the representatives of src's, in order, as codes, mapped to the caller's numbers
    void take_unique(Batch& dst, Batch& src, uint64_t* n_unique, uint64_t* bases_kept, float* device_ms);
    void download(std::vector<uint64_t>& read, std::vector<uint64_t>& rep) const;
    // dst := as after reset(src.n_reads), then for every entry j the records src holds for rep[j], numbered read[j]
    void expand(Fold& dst, Fold& src, float* device_ms) const;
};

}  // namespace mtsv

struct mtsv_dupmap {
    mtsv::DupMap impl;
    explicit mtsv_dupmap(int device) : impl(device) {}
};
