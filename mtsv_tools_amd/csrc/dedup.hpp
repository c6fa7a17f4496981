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
    DevBuf<uint32_t> d_read[2], d_rep[2];  // the same capacity each
    int cur = 0;
    bool valid = false;  // a take has succeeded
    uint64_t n = 0, n_unique = 0;
    // scratch of a take
    DevBuf<uint64_t> d_hash, d_table, d_words, d_ctr;
    DevBuf<uint32_t> d_slot;
    DevEvents<8> ev;
    float ms_hash = 0, ms_insert = 0, ms_resolve = 0, ms_scan = 0, ms_copy = 0;  // of the last take
    // scratch of an expansion (the map itself is not changed by one)
    struct Fan {
        DevBuf<uint32_t> d_first, d_cnt, d_off;  // n, n, n + 1 entries
        DevBuf<uint64_t> d_sums;                 // the scan's tile sums, then (at sums_cap) its total, then the counter
        uint64_t sums_cap = 0;
        DevEvents<4> ev;  // around count + scan, around write
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
