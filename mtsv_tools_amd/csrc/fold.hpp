// fold.hpp -- an accumulator of assignment records in HBM that outlives the workspaces whose runs are folded into it (fold.hip).
#pragma once
#include <memory>
#include <vector>

#include "../../include/mtsv_amd.h"
#include "abund.hpp"
#include "batch.hpp"
#include "lca.hpp"
#include "pair.hpp"
#include "parse.hpp"
#include "text.hpp"

namespace mtsv {

// The sorted union of the assignment lists folded so far, one record per key (k_fold.hip), in one of two arrays that take
// turns: a fold reads the current one and the incoming list and writes the other.  Bound to a device and a grain; it keeps
// no pointer to a workspace or an index.  What is counted per read -- the match flags, the taxa report -- is derived from
// the records when it is asked for.
struct Fold {
    int device;
    int grain;
    uint32_t tile = kFoldTile;  // MTSV_FOLD_TILE, read at creation (tests)
    bool trace = false;
    hipStream_t stream = nullptr;
    DevEvents<2> ev;
    DevBuf<uint8_t> d_rec[2];  // cap records each; they grow together (stage_write, commit)
    uint64_t cap = 0, n = 0;
    int cur = 0;
    DevBuf<uint8_t> d_in;  // the incoming list: a run's records gathered from its lanes' arrays, or uploaded ones
    DevBuf<uint32_t> d_tile_cnt, d_tile_off;
    DevBuf<uint64_t> d_tile_sums;  // the scan's tile sums, then (at sums_cap) its total
    uint64_t sums_cap = 0;
    uint64_t n_reads = 0;             // the caller's numbering (reset)
    std::vector<uint32_t> taxa;       // the TaxIDs of every source folded so far, ascending
    DevBuf<uint64_t> d_flags;         // flag words, then two counters
    DevBuf<uint32_t> d_taxa;
    DevBuf<uint64_t> d_counts;
    uint32_t text_tile = kTextTile;       // MTSV_TEXT_TILE, read at creation (tests)
    std::unique_ptr<TextFormatter> text;  // created by the first format_text
    uint32_t parse_tile = kParseTile;     // MTSV_PARSE_TILE, read at creation (tests)
    std::unique_ptr<TextParser> parser;   // created by the first add_text
    uint32_t lca_tile = kLcaTile;         // MTSV_LCA_TILE, read at creation (tests)
    std::unique_ptr<LcaState> lca_state;  // created by the first lca
    uint32_t pair_tile = kPairTile;          // MTSV_PAIR_TILE, read at creation (tests)
    uint32_t pair_lane_max = kPairLaneMax;   // MTSV_PAIR_LANE_MAX, read at creation (tests): 0 sends every window to the wavefront tier
    std::unique_ptr<PairState> pair_state;   // created by the first pair
    uint32_t abund_tile = kAbundTile;            // MTSV_ABUND_TILE, read at creation (tests)
    uint32_t abund_lane_max = kAbundLaneMax;     // MTSV_ABUND_LANE_MAX, read at creation (tests): 0 sends every read to the wavefront tier
    uint32_t abund_dense_max = kAbundDenseMax;   // MTSV_ABUND_DENSE_MAX, read at creation: the largest union whose adds go through LDS; 0: none
    uint64_t abund_start_mass = 1ull << 32;      // MTSV_ABUND_START_MASS, read at creation (tests): A_0 of an entering TaxID, 1 .. 2^32
    std::unique_ptr<AbundState> abund_state;     // created by the first abundance

    Fold(int device, int grain);
    ~Fold();
    Fold(const Fold&) = delete;
    Fold& operator=(const Fold&) = delete;

    uint64_t rec_bytes() const { return grain == MTSV_GRAIN_TAXID ? sizeof(mtsv_assignment) : sizeof(mtsv_assignment_gi); }
    void reset(uint64_t n_reads);
    void add_run(Batch& src, float* device_ms);
    void add_records(const void* records, uint64_t n, float* device_ms);
    // the hit parts of result lines, parsed on the device (parse.hip) and folded like a run's list
    void add_text(const char* hits, const uint64_t* line_off, const uint32_t* line_read, uint64_t n_lines, uint64_t* n_tokens, uint64_t* n_records,
                  float* device_ms);
    void download(void** a, uint64_t* n, bool wide);
    void taxa_report(std::vector<mtsv_taxon_stats>& rows, uint64_t* total_reads, float* device_ms);
    void match_flags(std::vector<uint64_t>& words, uint64_t* n_reads, uint64_t* n_matched);
    // the result lines of the accumulated records, written on the device (text.hip); the fold is not changed
    void format_text(const char* ids, const uint64_t* id_off, uint64_t n_reads, char** text, uint64_t* len, float* device_ms);
    // per read with a record the LCA of its taxa within edit_slack of its smallest edit (lca.hip, k_lca.hip): one record
    // (read, LCA TaxID, smallest edit) per read into `out` (may be null; a fold of this device at MTSV_GRAIN_TAXID, not this
    // one), which becomes as after reset(n_reads) with those records; the clade rows in preorder (rows may be null); this
    // fold is not changed
    void lca(const Taxonomy& tx, uint32_t edit_slack, Fold* out, std::vector<mtsv_clade_stats>* rows, uint64_t* total_reads, float* device_ms);
    // reads 2p and 2p + 1 are the mates of pair p: one record (p, TaxID, edit) per TaxID the mode keeps for the pair (pair.hip,
    // k_pair.hip) into `out` (a fold of this device at MTSV_GRAIN_TAXID, not this one), which becomes as after reset(n_reads / 2)
    // with those records and this fold's TaxID union; stats may be null; this fold is not changed
    void pair(int mode, uint32_t max_insert, uint32_t unpaired_edits, Fold* out, mtsv_pair_stats* stats, float* device_ms);
    // abundance by expectation-maximisation over the reads' entering taxa (abund.hip, k_abund.hip; the definition is in
    // include/mtsv_amd.h): one record (read, assigned TaxID, its smallest edit) per read into `out` (may be null; a fold of this
    // device at MTSV_GRAIN_TAXID, not this one), which becomes as after reset(n_reads) with those records; a row per entering
    // TaxID (rows and info may be null); this fold is not changed
    void abundance(const uint32_t* w, uint32_t n_w, uint32_t edit_slack, uint32_t max_iters, uint64_t tol, Fold* out, std::vector<mtsv_abundance_row>* rows,
                   mtsv_abundance_info* info, float* device_ms);

    // A write of a whole new record list (fold_in, lca, pair, DupMap::expand) is staged: dst is the array that is not current, or,
    // when that is too small, the first of a new pair, which the fold takes only with commit.  A Staged that is not
    // committed frees its pair; one that is frees the pair the fold had.
    struct Staged {
        uint8_t* dst = nullptr;
        DevBuf<uint8_t> pair[2];
        uint64_t cap = 0;  // of the new pair, in records; 0: dst is the fold's other array
    };
    // room for n_records; throws "device: no memory for <what> of ... records (two arrays)" and leaves the fold as it was
    Staged stage_write(uint64_t n_records, const char* what);
    // the fold holds the n_records written at s.dst: cannot fail (the caller has waited for the writes)
    void commit(Staged& s, uint64_t n_records);

   private:
    void in_room(uint64_t n_b);
    // d_in[0 .. n_b) folded into the accumulator; new_taxa (ascending) joins the union when it has succeeded
    void fold_in(uint64_t n_b, std::vector<uint32_t>& new_taxa, float* device_ms);
};

}  // namespace mtsv

struct mtsv_fold {
    mtsv::Fold impl;
    template <class... A>
    explicit mtsv_fold(A&&... a) : impl(std::forward<A>(a)...) {}
};
