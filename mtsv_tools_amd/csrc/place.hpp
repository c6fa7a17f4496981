// place.hpp -- the alignments of a workspace's hits (place.hip, k_place.hip; mtsv_batch_place_hits, include/mtsv_amd.h).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mtsv_amd.h"
#include "dev_mem.hpp"
#include "kernels.hpp"

namespace mtsv {

struct Batch;

// Everything a call needs beside the workspace's reads, hits and index: the table of the index's bins by (tax_id, gi), the
// gathered hits, the scratch of the map pass, the ring and the two result arrays.  A workspace creates one on its first call
// and keeps it; the arrays grow by reallocation and are kept from call to call.  It works on the workspace's own stream.
struct Placer {
    int device;
    bool trace = false, timing = false;
    uint32_t ring_env = 0;                // MTSV_PLACE_RING, read at creation (tests): columns of the ring, forced up to what a call needs
    uint64_t ring_budget = 1ull << 30;    // bytes of ring a call may hold: fewer lanes stride the hits when a lane's ring is large
    DevEvents<5> ev;
    // the table: built by the first call (the workspace's index never changes)
    bool table_ready = false;
    uint32_t n_keys = 0;
    DevBuf<uint64_t> d_key;
    DevBuf<uint32_t> d_bin_of_key;
    // of a call
    DevBuf<DevHit> d_in;                        // the hits, next to each other
    DevBuf<uint32_t> d_hit_bin, d_hit_read, d_cnt, d_off;  // by hit (off: n + 1)
    DevBuf<uint64_t> d_sums, d_ctr;             // the scan's tile sums; kPlaceCounters, then the scan's total
    DevBuf<uint32_t> d_ring, d_ops;
    DevBuf<uint8_t> d_out;                      // n placements of 48 bytes

    explicit Placer(int device);
    Placer(const Placer&) = delete;
    Placer& operator=(const Placer&) = delete;

    // what a placement left on the device: n placements in d_out (hit k of d_in, with d_hit_bin[k] and d_hit_read[k]), their
    // ops in d_ops[0 .. total_ops)
    struct Placed {
        uint64_t n = 0, total_ops = 0, span = 0, columns = 0;
        bool own = false;
        uint32_t words = 0, cols = 0, blocks = 0;
        float ms_map = 0, ms_place = 0;
    };

    void place(Batch& b, const mtsv_hit* hits, uint64_t n_hits, mtsv_placement** out, uint64_t* n_out, uint32_t** ops, uint64_t* n_ops_total,
               float* device_ms);
    // place() without its copies to the host: every refusal of place(), then placements and ops valid on the device and the
    // stream idle.  r.n == 0: nothing was launched.
    void place_on_device(Batch& b, const mtsv_hit* hits, uint64_t n_hits, Placed& r);

   private:
    void build_table(Batch& b);
    void map_hits(Batch& b, const mtsv_hit* hits, uint64_t n_hits, Placed& r);
    void place_mapped(Batch& b, Placed& r);
    mtsv_hit hit_at(uint64_t k) const;
};

}  // namespace mtsv
