// abund.hpp -- what a fold keeps for mtsv_fold_abundance (abund.hip): the arrays of a call.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "dev_mem.hpp"
#include "kernels.hpp"

namespace mtsv {

// Created by a fold's first abundance call, on the fold's stream.  Nothing is kept between calls but the room: up to 29 bytes
// per record of the fold, 28 per read with a record and 32 per TaxID of the union.
struct AbundState {
    int device;
    hipStream_t stream;  // the fold's
    bool timing = false;
    uint32_t cus = 1;  // the device's compute units: the persistent kernels' grids
    DevEvents<9> ev;
    DevBuf<uint32_t> d_tile;    // cnt_r, cnt_p (tiles each), off_r, off_p (tiles + 1 each)
    DevBuf<uint64_t> d_sums;    // the scans' tile sums
    DevBuf<uint64_t> d_ctr;     // kAbundCounters, then the three scans' totals, then L1
    DevBuf<uint64_t> d_read64;  // read_id (n_reads)
    DevBuf<uint32_t> d_read32;  // m, read_first, list (n_reads each), read_off (n_reads + 1)
    DevBuf<uint32_t> d_run32;   // e_run, run_tax, run_read, flag (n_runs each), off (n_runs + 1)
    DevBuf<uint32_t> d_ent32;   // ent_slot, ent_e (n_runs each: the entries are at most the runs)
    DevBuf<uint8_t> d_ent8;     // ent_d
    DevBuf<uint32_t> d_tax32;   // u_tax, any, uniq, assigned (n_union each), w (256)
    DevBuf<uint64_t> d_mass;    // mass, next (n_union each)
    DevBuf<uint8_t> d_out;      // the records of a call without an output fold

    AbundState(int device, hipStream_t stream);
    ~AbundState();
    AbundState(const AbundState&) = delete;
    AbundState& operator=(const AbundState&) = delete;
};

}  // namespace mtsv
