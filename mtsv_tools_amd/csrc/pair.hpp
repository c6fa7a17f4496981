// pair.hpp -- what a fold keeps for mtsv_fold_pair (pair.hip): the arrays of a call.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "dev_mem.hpp"
#include "kernels.hpp"

namespace mtsv {

// Created by a fold's first pair call, on the fold's stream.  The arrays grow by reallocation and are kept.
struct PairState {
    int device;
    hipStream_t stream;  // the fold's
    bool timing = false;
    DevEvents<8> ev;
    DevBuf<uint32_t> d_off;                   // the reads' first records: n_reads + 1
    DevBuf<uint32_t> d_val, d_add;            // by record; then the slots' flags for list A and list B
    DevBuf<uint32_t> d_list;                  // the work list of the wavefront tier (n + 1); then the scan of list A's flags
    DevBuf<uint32_t> d_pos_b;                 // the scan of list B's flags (n + 1)
    DevBuf<uint32_t> d_m;                     // by slot: the run's minimum, then its value
    DevBuf<uint4> d_slot;                     // by slot: (read, tax_id, add)
    DevBuf<uint32_t> d_tile_cnt, d_tile_off;  // of the heads, then of the merge of the two lists
    DevBuf<uint64_t> d_sums;                  // the scans' tile sums
    DevBuf<uint64_t> d_ctr;                   // kPairCounters, then the scans' totals: slots, list A, list B, merged
    DevBuf<uint8_t> d_lists;                  // list A, then list B (MTSV_PAIR_EITHER)

    PairState(int device, hipStream_t stream);
    ~PairState();
    PairState(const PairState&) = delete;
    PairState& operator=(const PairState&) = delete;
};

}  // namespace mtsv
