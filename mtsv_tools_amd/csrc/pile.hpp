// pile.hpp -- the accumulator of a pileup per reference position (pile.hip, k_pile.hip; mtsv_pileup, include/mtsv_amd.h).
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/mtsv_amd.h"
#include "dev_mem.hpp"
#include "kernels.hpp"
#include "pile_refs.hpp"

namespace mtsv {

struct Batch;

// Bound to a device and a list of TaxIDs.  The references it has met lie in SEGMENTS, one per call that brought new ones; a
// segment's arrays are allocated once and never moved.  add_run works on the workspace's stream and leaves it idle; sites,
// download and reset work on a stream of the accumulator's own.
struct Pileup {
    struct Segment {
        uint32_t n_slots = 0, n_refs = 0;
        DevBuf<uint32_t> cnt;       // [slot][8], channel 0 a difference array
        DevBuf<uint8_t> ref;        // the text's code per slot, 0xff for a reference's last slot
        DevBuf<uint32_t> ref_off;   // n_refs + 1
        DevBuf<uint64_t> ref_key;   // n_refs
        uint64_t bytes() const { return (uint64_t)n_slots * 33 + ((uint64_t)n_refs + 1) * 4 + (uint64_t)n_refs * 8; }
    };
    int device;
    DevStream stream;
    bool trace = false, timing = false;
    uint32_t tile = kPileTile;  // MTSV_PILE_TILE, read at creation (tests)
    bool cons_staged = kConsStagedDefault;  // MTSV_CONS_WRITE=plain|staged, read at creation (tests, tools/cons_ab.py)
    DevEvents<10> ev;
    PileRefs refs;
    std::vector<std::unique_ptr<Segment>> segs;
    uint64_t hits_piled = 0, hits_skipped = 0;
    // of a call
    std::vector<uint32_t*> h_bin_cnt;
    DevBuf<uint32_t*> d_bin_cnt;
    DevBuf<uint32_t> d_best;
    DevBuf<uint64_t> d_ctr, d_sums;
    DevBuf<uint32_t> d_tile_sum, d_tile_pre, d_tile_cnt, d_tile_off, d_dump;
    DevBuf<uint8_t> d_rows;
    // of a consensus call (cons.hip)
    DevBuf<uint8_t> d_call, d_text;
    DevBuf<uint32_t> d_cells, d_ref_pre, d_lay, d_add;

    Pileup(int device, const uint32_t* taxa, uint64_t n_taxa);
    ~Pileup();
    Pileup(const Pileup&) = delete;
    Pileup& operator=(const Pileup&) = delete;

    void reset();
    void add_run(Batch& b, const mtsv_hit* hits, uint64_t n_hits, uint32_t edit_slack, uint64_t* n_piled, uint64_t* n_skipped, float* device_ms);
    void info(mtsv_pileup_info_t* out) const;
    void download(uint32_t tax_id, uint32_t gi, std::vector<uint32_t>& counts, std::vector<uint8_t>& ref);
    void sites(uint32_t min_depth, uint32_t min_alt, uint32_t min_alt_ppm, std::vector<mtsv_pile_site>& rows, float* device_ms);
    // cons.hip.  fasta == nullptr: rows only, no layout and no write kernel
    void consensus(uint32_t min_depth, uint32_t min_frac_ppm, uint32_t min_breadth_ppm, uint32_t fill, uint32_t line_width, std::vector<char>* fasta,
                   std::vector<mtsv_cons_ref>& rows, float* device_ms);
    void add_counts(uint32_t tax_id, uint32_t gi, uint32_t first_slot, uint64_t n_slots, const uint32_t* counts, uint64_t n_hits);

   private:
    std::unique_ptr<Segment> make_segment(Batch& b, const PileRefs::Plan& plan);
    void integrate(Segment& sg);  // d_tile_pre = the match depth in front of every tile of the segment
};

}  // namespace mtsv

struct mtsv_pileup {
    mtsv::Pileup impl;
    mtsv_pileup(int device, const uint32_t* taxa, uint64_t n_taxa) : impl(device, taxa, n_taxa) {}
};
