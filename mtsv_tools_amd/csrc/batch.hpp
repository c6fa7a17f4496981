// batch.hpp -- device workspace of one read batch (see batch.hip; the pass driver: batch_pass.hip; the host run: batch_host.hip).
#pragma once
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/mtsv_amd.h"
#include "host_pack.hpp"
#include "dev_index.hpp"
#include "dev_mem.hpp"
#include "kernels.hpp"

namespace mtsv {

// result arrays in pinned host memory, recycled through a pool (mtsv_hits_free returns them)
mtsv_hit* pinned_hits_alloc(uint64_t n_hits, uint64_t* cap_hits);
bool pinned_hits_release(void* p);  // false: p is not a pool array

// A pool array that a host run fills in read order while later ranges still compute -- the hits, the assignments -- and that
// the download then hands to the caller as it is.  The pool counts in 32-byte hits: records of `rec` bytes are rounded up to
// those units on the way in and the capacity is turned back into records on the way out; with 32-byte hits both are the
// identity, so one body gives both arrays the sizes they had with one body each.
struct PinnedStage {
    uint8_t* p = nullptr;
    uint64_t cap = 0, staged = 0;  // records the array holds; records copied into it so far
    uint64_t rec;                  // bytes per record
    uint64_t last_total = 0;       // records of the last run that was downloaded: what begin() expects of the next
    bool valid = false;            // the last run staged all of its records
    const char *name, *unit;       // (trace)
    PinnedStage(uint64_t rec_, const char* name_, const char* unit_) : rec(rec_), name(name_), unit(unit_) {}
    PinnedStage(const PinnedStage&) = delete;
    PinnedStage& operator=(const PinnedStage&) = delete;
    ~PinnedStage() { drop(); }
    // an array if there is none, for about the records of the last run (first run: expected_first)
    void begin(uint64_t expected_first);
    // room for `need` records: after `stream` is through with the old array a larger one takes over what has been staged
    void reserve(uint64_t need, hipStream_t stream);
    uint8_t* at(uint64_t record) const { return p + record * rec; }
    void* hand_out();  // the array is the caller's; the stage holds nothing
    void drop();       // the array goes back to the pool
};

struct Batch {
    mtsv_index* ix;
    DeviceIndex* di;
    // Every resource is a member that frees itself (dev_mem.hpp; DESIGN.md, "The host side of the stages behind the binner"),
    // the streams first, so that they are destroyed after the arrays.  copy_stream (the reads' transfer) and copy_stream2
    // (results to the host) are created by the first host batch, at high priority (host_room).
    DevStream stream, copy_stream, copy_stream2;
    PinnedStage hits_stage{sizeof(mtsv_hit), "result", "hits"};  // run_host copies every range's hits here while later ranges run
    // run_host: the input arenas in HBM (the whole host batch, or segments of it taking turns), filled in read order by one
    // feeder thread on copy_stream; page-locked staging chunks for bases that lie in ordinary memory
    struct Arena {
        DevBuf<uint8_t> d_bases;
        DevBuf<uint8_t> d_packed;  // the same bases as they arrive: 4-bit codes, two per byte (host_pack.hpp)
        DevBuf<uint32_t> d_off;
        uint64_t cap_bases = 0, cap_reads = 0;  // above zero: the three arrays exist at these sizes
        void resize(int k, uint64_t bases, uint64_t reads);  // contents not kept
    };
    static constexpr uint64_t kArenaBases = 3ull << 30;   // offsets inside a segment are u32
    static constexpr uint64_t kArenaReads = 1ull << 30;
    Arena arena[2];
    HostBuf<uint32_t> h_off_all;  // pinned: the batch's offsets, narrowed to segment-relative u32
    static constexpr int kStage = 4;
    HostBuf<uint8_t> h_stage[kStage];
    DevEventList chunk_ev;  // one per copy chunk (hipEventDisableTiming), kept between runs
    std::mutex* commit_mu = nullptr;  // set while run_host's threads may touch the lanes' result arrays (HostRun::run_threads)
    uint64_t max_reads, max_bases;
    // entries of each of the ten seed-hit arrays (d_hit_row .. d_worklist).  Above zero: all ten exist at that size, on every
    // path; zero after a growth that failed, and then the next run begins with the first size again (hit_cap_first)
    uint64_t hit_cap, hit_cap_first = 0;
    // Lanes: the workspace is cut into n_lanes equal parts, each with its own stream; a resident range of
    // reads is split across them and the parts run concurrently (one host thread each), so that the
    // HBM-latency-bound stages of one part overlap the VALU-bound verification of another.  The owner
    // is lane 0 and holds the input buffers; the other lanes borrow them.  MTSV_LANES=1 disables it.
    Batch* parent = nullptr;
    Batch* root() { return parent ? parent : this; }  // the owner: turn, report, flags, assignments and lane policies are its
    const Batch* root() const { return parent ? parent : this; }
    std::vector<std::unique_ptr<Batch>> extra;
    int n_lanes = 1;
    uint64_t ws_reads = 0;  // reads one lane's workspace is sized for
    struct Segment {
        Batch* lane;
        uint64_t offset, count;
        uint64_t first_read = 0, n_reads = 0;  // (resident runs) the range of the batch's reads whose hits these are
        uint64_t a_offset = 0, a_count = 0;    // (assignments on) the same stretch's assignments in the lane's d_assign
    };
    std::vector<Segment> segments;  // where the hits of the last run sit, in read order
    uint64_t total_hits = 0;
    double run_t0 = 0;
    uint64_t lanes_used = 1;

    // (the owner's; empty in the other lanes, which borrow them)
    DevBuf<uint8_t> d_codes;  // run(): normalised copy of d_bases
    DevBuf<uint8_t> d_bases;  // resident batch of upload() / run()
    DevBuf<uint32_t> d_read_off;
    DevBuf<uint32_t> d_seed_lo, d_seed_cnt, d_seed_pre;
    uint64_t seed_cap = 0;  // above zero: the three seed slot arrays exist at that size
    DevBuf<uint32_t> d_strand_hits, d_strand_nseeds, d_strand_off, d_strand_ncand, d_worklist, d_strand_nout, d_out_off;
    DevBuf<uint64_t> d_tile_sums;
    DevBuf<uint64_t> d_counters;
    DevBuf<uint32_t> d_hit_row, d_hit_ref, d_hit_q;
    DevBuf<uint64_t> d_hit_key, d_cand_tmp;
    DevBuf<uint4> d_cand, d_out;
    DevBuf<uint32_t> d_cand_next, d_cand_status, d_heavy_list;
    DevBuf<DevHit> d_hits;    // grows keeping its contents (room_hits)
    DevBuf<uint2> d_strip;    // tiled long-read kernel: band hand-over strips, allocated when a pass first needs them
    DevBuf<uint32_t> d_planes;  // bit planes of a pass's reads (EvalArgs::planes): k_thin writes them, k_edit_myers sets up from them;
                                // in words, allocated when a pass first needs them, for a full workspace of such reads
    HostBuf<uint64_t> h_counters;  // pinned, mapped
    enum Ev {
        // a pass: stage s (MTSV_N_STAGES' first seven) lies between events s and s + 1
        kEvPassBegin = 0, kEvSearched, kEvSeeded, kEvExpanded, kEvLocated, kEvCoalesced, kEvVerified, kEvGathered,
        kEvRunBegin, kEvRunEnd,  // the lane's run
        kEvSwBegin, kEvSwEnd,    // round 0: around the prefilter kernels
        kEvDiagEnd,              // ... after k_sw_diag
        kEvBoundEnd,             // ... after the edit-distance bound
        kEvEditEnd,              // ... after its edit distances
        kEvCount
    };
    DevEvents<kEvCount> ev;
    float sw_ms_acc = 0, sweep_ms_acc = 0, diag_ms_acc = 0, bound_ms_acc = 0, edit_ms_acc = 0;
    uint64_t sw_passed_acc = 0;   // candidates k_sw_pairs sent on to the edit distance (all rounds and passes of the run)

    std::vector<uint32_t> h_read_off;
    uint32_t max_len = 0;
    static constexpr int kCounters = kCtrCount;  // (the slots: kernels.hpp)
    double listed_share = 0.125;  // seed slots that took the general search code in the last pass, with a margin (k_search_listed's grid)
    bool sw_diag = true;   // k_sw_pairs tries the ungapped diagonal as a lower bound first (MTSV_SW_DIAG=0: off)
    bool sw_top = true;      // ... and what they leave is swept on the top half of the read rows first (MTSV_SW_TOP=0: off)
    bool sw_bound = true;    // ... first by the edit-distance bound on the score (k_edit_myers in bound mode; MTSV_SW_BOUND=0: off)
    bool sw_fused = true;    // ... and that pass decides the edit distance too, on the whole worklist, with no k_sw_diag before it (MTSV_SW_FUSED=0: off)
    bool sw_prepass = true;  // the first round's bounds run as a kernel of their own, k_sw_diag (MTSV_SW_PREPASS=0: inside k_sw_pairs)
    bool sw_pairs = true;  // reference order for reads <= 253 bases: k_sw_pairs + k_edit_myers (MTSV_SW=packed: k_evaluate)
    // Lane policies, read from the environment when the owner is created and handed to its lanes ("Lanes"):
    uint32_t myers_wgs_per_cu = kMyersWgsPerCuMax;  // k_edit_myers' grid is 256 x this many workgroups at most: five fill a CU's LDS, a workspace
                                                    // of several lanes leaves room for the other lanes' kernels (MTSV_MYERS_WGS_PER_CU)
    bool tail_from_list = true;  // round 0's k_sw_pairs and list-mode k_edit_myers are sized from the undecided count the fused pass
                                 // publishes, and not launched when it is zero (MTSV_TAIL_FROM_LIST=0: sized from the seed hits)
    bool fused_clear = true;     // the counters of a stage are zeroed by one launch_clear_counters (MTSV_FUSED_CLEAR=0: a memset each)
    bool seed_tiles = true;      // the seed stage by tiles, k_thin_tiled + k_expand_tiled, for the passes that fit them (MTSV_SEED_STAGE=legacy:
                                 // k_thin writing seed_pre and k_expand reading it, for every pass)
    bool myers_fetch_legacy = false;  // k_edit_myers fetches its windows lane by lane, 16 columns at a time, and not by quads and whole
                                      // sectors (MTSV_MYERS_FETCH=legacy)
    bool listed_zero = false;    // ... kCtrListedSlots (k_search's list count) is known to be zero on the stream
    // The verify turn: one lane of a workspace at a time has the verify kernels of a pass in flight (two VALU-bound launches beside
    // each other gain nothing, and the second takes the LDS the first frees from the memory-bound kernels that could use it).  The
    // owner holds it; lanes waiting for it are served in the order of their passes' first reads (MTSV_VERIFY_TURN=0: off; never
    // used by a workspace of one lane).
    struct VerifyTurn {
        bool on = false;
        std::mutex mu;
        std::condition_variable cv;
        bool held = false;
        std::vector<std::pair<uint64_t, const Batch*>> waiting;
        // of the last run (mtsv_batch_stats): passes that took the turn; lanes inside the verify section of a pass at once, at
        // most (counted with the turn on or off: 1 shows that it serialises); the largest k_edit_myers grid launched
        uint64_t taken = 0, in_verify = 0, max_in_verify = 0, myers_grid_max = 0;
        void enter(uint64_t first_read, const Batch* lane);  // waits for the turn when it is on
        void leave();
        void note_grid(uint32_t blocks);
        // holds the turn from take() until release() or the end of the scope, whichever comes first
        struct Guard {
            VerifyTurn* t = nullptr;
            Guard() = default;
            Guard(const Guard&) = delete;
            Guard& operator=(const Guard&) = delete;
            ~Guard() { release(); }
            void take(VerifyTurn& turn, uint64_t first_read, const Batch* lane) {
                if (t) return;
                turn.enter(first_read, lane);
                t = &turn;
            }
            void release() {
                if (t) t->leave();
                t = nullptr;
            }
        };
    };
    VerifyTurn verify_turn;
    int verify_mode = 0;  // 0 = reference order (SW + edit per candidate), 1 = edit first (MTSV_VERIFY_EDIT_FIRST)
    uint64_t n_reads = 0;
    uint64_t n_hits_total = 0;
    mtsv_batch_stats stats{};
    float stage_acc[MTSV_N_STAGES] = {0};

    // lanes: ranges of a host batch that run through the kernels at once, each on a stream and workspace of its own (0: three,
    // MTSV_LANES)
    Batch(mtsv_index* ix, DeviceIndex* di, uint64_t max_reads, uint64_t max_bases, uint64_t hit_cap, Batch* parent = nullptr, int lanes = 0);
    ~Batch();
    Batch(const Batch&) = delete;
    Batch& operator=(const Batch&) = delete;

    void upload(const uint8_t* bases, const uint64_t* read_off, uint64_t n);
    void run(const mtsv_params& p);
    // read_base: added to the `read` field of every hit (a caller that shards one host batch over devices)
    void run_host(const uint8_t* bases, const uint64_t* read_off, uint64_t n, const mtsv_params& p, uint64_t read_base = 0);
    struct HostPart {
        const uint8_t* bases;
        const uint64_t* read_off;  // n + 1 offsets into bases
        uint64_t n;
    };
    void run_host_parts(const HostPart* parts, int n_parts, const mtsv_params& p, uint64_t read_base = 0);
    // everything run_host sizes by the batch it is given (device arenas, offset table, result array), for batches of up to
    // n reads / n_bases bases, now
    void reserve_host(uint64_t n, uint64_t n_bases);
    void download(mtsv_hit** hits, uint64_t* n);
    // the hits of the last run, still in HBM (keep_on_device was set), into caller memory that holds n == total_hits entries
    void download_into(mtsv_hit* dst, uint64_t n);
    bool keep_on_device = false;  // run_host: leave the hits in the lanes' result arrays (no copy to the host while it runs)

    // Taxa report (k_report.hip): per-TaxID read counts, added to by every committed pass of every lane while it is on.
    // Everything belongs to the owner and is created when the report is first switched on.
    struct TaxaReport {
        bool on = false;
        bool dense = true;
        uint32_t hash_slots = kReportHashSlots;  // of the hashed tier's LDS table (MTSV_REPORT_HASH_SLOTS: fewer, tests)
        uint32_t n_taxa = 0;
        DevBuf<uint32_t> d_taxa;    // the index's distinct TaxIDs, ascending
        DevBuf<uint64_t> d_counts;  // 4 per taxon (only_hit, only_best, tied_best, not_best), then the reads with a hit,
                                       // then (trace) the atomic adds the kernels made on all of these
        bool trace = false;            // MTSV_TRACE was set when the report was switched on
        uint64_t launches = 0;         // (under mu) report kernels since the last reset
        std::vector<uint32_t> h_taxa;
        std::mutex mu;                 // ms (the lanes' threads add to it)
        float ms = 0;                  // device time of the report kernels since the last reset
    };
    TaxaReport report;
    DevEvents<2> report_ev;  // around a lane's report kernel; created with the lane's first one
    void set_taxa_report(bool on);
    // Match flags (k_match.hip): one bit per read of the last run, "the run returned a hit for it".  Like the report they
    // belong to the owner; unlike it they describe one run: zeroed when a run begins, sized with it.
    struct MatchFlags {
        int mode = MTSV_MATCH_OFF;
        DevBuf<uint64_t> d_words;  // cap_words() words of flags, then the matched-reads counter
        uint64_t cap_words() const { return d_words.p ? d_words.cap - 1 : 0; }
        uint64_t n_reads = 0;         // of the last run with the flags on
        uint64_t call_base = 0;       // read_base of that run: bit 0 is its first read
        bool trace = false;
        std::mutex mu;                // ms, launches (the lanes' threads add to them)
        float ms = 0;                 // device time of the run's k_match launches
        uint64_t launches = 0;
    };
    MatchFlags match;
    DevEvents<2> match_ev;  // around a lane's k_match; created with the lane's first one
    bool flags_only() const { return root()->match.mode == MTSV_MATCH_ONLY; }
    void set_match_flags(int mode);
    // the flags of the last run as ceil(n_reads / 64) words (at least one), bits at and above n_reads zero
    void match_flags(std::vector<uint64_t>& words, uint64_t* n_reads, uint64_t* n_matched);
    // Chaining (k_compact.hip): the reads of src's last run whose match flag is clear (keep = MTSV_KEEP_UNMATCHED) or set become
    // this workspace's resident batch, as codes, with a map to the caller's read numbers.  All of it belongs to the owner
    // and is created by the first take_reads.
    enum LastRun { kRunNone = 0, kRunResident, kRunHostOneSegment, kRunHostSegments, kRunMerged };
    int last_run = kRunNone;       // what the last completed run left in HBM (a source of take_reads needs its reads)
    bool resident = false;         // upload() or take_reads() filled the resident batch, no host batch has run since
    bool codes_resident = false;   // ... take_reads did: d_codes holds it (d_bases does not), run() must not normalise
    bool mapped = false;           // ... and d_read_map translates its read numbers in every gathered hit
    DevBuf<uint32_t> d_read_map;   // max_reads entries
    DevBuf<uint64_t> d_compact;    // the result block (3 words), then two arrays of tile sums
    uint64_t compact_cap() const { return d_compact.p ? (d_compact.cap - 3) / 2 : 0; }  // ... entries each
    DevEvents<4> compact_ev;  // around the scan and around the copy
    void compact_room(uint64_t tiles);  // d_compact for that many tiles, and d_read_map; on the workspace's device
    void take_reads(Batch& src, int keep, uint64_t* n_kept, uint64_t* bases_kept, float* device_ms);
    // this workspace's resident batch := a copy of src's (codes or bases, offsets, longest read, read map), HBM to HBM
    void copy_reads(Batch& src, float* device_ms);
    // Merging (k_merge.hip): the last runs of srcs[0 .. n_srcs), which hold the same reads, merged per read into this
    // workspace's result array, laid out as one pass; the report and the flags, where on, take the merged reads.  All of
    // it belongs to the owner and is created by the first merge_runs.
    struct MergeState {
        DevBuf<uint32_t> d_nout, d_off;  // 2 n + 1 entries each
        DevBuf<uint64_t> d_tiles;        // the scan's cap_tiles() tile sums, then its total, then the copy's dropped hits
        uint64_t cap_reads = 0;          // above zero: d_nout, d_off and d_tiles exist for that many reads
        uint64_t cap_tiles() const { return d_tiles.cap - 2; }
        DevBuf<uint32_t> d_lo, d_base;   // per (source, read)
        uint64_t cap_sn = 0;             // above zero: both exist at that size
        DevBuf<MergePart> d_parts;
        DevEvents<2> ev;
    };
    MergeState merge;
    // Assignments (k_collapse.hip): per read of the last run one (read, tax_id, smallest edit) record per distinct TaxID,
    // ascending by TaxID -- the default results line of mtsv-binner, reduced on the device.  The mode, the thresholds and the
    // times belong to the owner; every lane has a result array and a scratch of its own, created by its first pass with the
    // assignments on.  Like the flags they describe one run.  The grain (mtsv_batch_set_assignment_grain) decides what a
    // record is: MTSV_GRAIN_TAXID the 16-byte one above, MTSV_GRAIN_TAXID_GI and MTSV_GRAIN_LONG the 24-byte mtsv_assignment_gi,
    // one per (TaxID, GI) or per (TaxID, GI, offset).  It changes only while the mode is off, so the record arrays of a
    // workspace hold records of one size while they are in use; every count and offset of assignments is in records.
    struct Assignments {
        int mode = MTSV_ASSIGN_OFF;
        int grain = MTSV_GRAIN_TAXID;
        uint64_t rec_bytes() const { return grain == MTSV_GRAIN_TAXID ? sizeof(mtsv_assignment) : sizeof(mtsv_assignment_gi); }
        uint64_t key_bytes() const { return grain == MTSV_GRAIN_TAXID ? 8 : 16; }
        // a read of up to lane_max hits is reduced by one lane, up to wave_max by its wavefront, up to lds_max by a workgroup
        // in LDS, a larger one by a workgroup in global memory (MTSV_COLLAPSE_LANE_MAX, _WAVE_MAX, _LDS_MAX: tests)
        uint32_t lane_max = kCollapseLaneMax, wave_max = 64, lds_max = kCollapseLdsKeys;
        bool trace = false;
        std::mutex mu;          // ms, launches, tiers (the lanes' threads add to them)
        float ms = 0;           // device time of the run's collapse kernels
        uint64_t launches = 0;
        uint64_t tiers[5] = {0, 0, 0, 0, 0};  // reads of the run by tier: lane, wavefront, listed = LDS + global
    };
    Assignments assign;
    // run_host: a finished range's assignments leave for this pinned array (pool) on the result copy stream, in read order,
    // like its hits; mtsv_batch_download_assignments hands the array out.  (owner only)
    PinnedStage assign_stage{sizeof(mtsv_assignment), "assignment", "records"};  // records of assign.rec_bytes() (set_assignment_grain)
    bool host_hits_dropped = false;  // the last run was a host batch in MTSV_ASSIGN_ONLY: its hits were never staged and the lanes' arrays were recycled
    DevBuf<uint8_t> d_assign;  // the lane's assignments (records of the grain), those of a pass behind those of the passes before;
                               // grows keeping its contents (collapse_room)
    uint64_t n_assign_total = 0;
    struct CollapseScratch {
        DevBuf<uint64_t> keys;   // cap_hits sort keys of key_bytes each, mirroring a pass's hits
        uint64_t key_bytes = 0;
        DevBuf<uint32_t> flags, place;  // cap_hits + 1 each
        DevBuf<uint64_t> tiles;  // the scan's tile sums
        uint64_t cap_hits = 0;   // above zero: keys, flags, place and tiles exist for that many hits
        void resize(uint64_t hits, uint64_t key_bytes);  // contents not kept
        DevBuf<uint32_t> list;   // the reads left to k_collapse_heavy
        uint64_t pending_hits = 0;  // the hits of the pass whose collapse is on the stream
        DevBuf<uint64_t> d_ctr;  // kCollapseCounters
        HostBuf<uint64_t> h_ctr;  // pinned, mapped: the pass's counters (launch_publish)
        DevEvents<2> ev;
    };
    CollapseScratch collapse;
    bool assign_only() const { return root()->assign.mode == MTSV_ASSIGN_ONLY; }
    void set_assignments(int mode);
    void set_assignment_grain(int grain);
    // the assignments of the last run, in read order, in a pinned array of the pool (*n may be 0: *a is still to be freed)
    // (grain: the one the caller's record type belongs to -- MTSV_GRAIN_TAXID, or anything else for the 24-byte records)
    void download_assignments(void** a, uint64_t* n, float* device_ms, bool wide);
    // the result lines of the last run's assignments, written on the device (text.hip: mtsv_batch_format_text); the
    // formatter is created by the first call.  (owner only)
    std::shared_ptr<struct TextFormatter> text;
    void format_text(const char* ids, const uint64_t* id_off, uint64_t n_reads, char** text_out, uint64_t* len, float* device_ms);
    // the alignments of hits against the resident batch (place.hip: mtsv_batch_place_hits) -- of the last run's hits where they
    // lie in HBM (hits null), or of n_hits given ones; the placer is created by the first call.  (owner only)
    std::shared_ptr<struct Placer> placer;
    void place_hits(const mtsv_hit* hits, uint64_t n_hits, mtsv_placement** out, uint64_t* n_out, uint32_t** ops, uint64_t* n_ops_total, float* device_ms);
    void merge_runs(Batch* const* srcs, int n_srcs, float* device_ms);
    void read_map(std::vector<uint64_t>& map);
    void download_reads(std::vector<uint8_t>& codes, std::vector<uint64_t>& read_off);
    // rows: every TaxID with a non-zero counter, ascending
    void taxa_report(std::vector<mtsv_taxon_stats>& rows, uint64_t* total_reads, float* device_ms, bool reset);

   private:
    void begin_run(const mtsv_params& p, uint64_t read_base = 0);
    void match_begin(uint64_t n, uint64_t read_base);  // flags on: room for n reads' flags, all zero
    void report_extend(Batch* const* srcs, int n_srcs);  // the report's TaxID list := its union with the sources' indexes
    // room for a pass of n_reads reads and n_hits hits in the lane's collapse scratch and behind its assignments so far
    void collapse_room(uint64_t n_reads, uint64_t n_hits);
    // (assignments on) the collapse of a committed pass on the lane's stream, its counters published; collapse_commit, after
    // the stream has been synchronised, takes them: returns the pass's assignments, now part of d_assign
    void collapse_enqueue(uint32_t n_reads, const uint32_t* strand_nout, const uint32_t* out_off, const DevHit* hits, uint64_t n_hits);
    uint64_t collapse_commit();
    void collapse_begin();  // a run begins: no assignments, counts and times zero
    void collapse_trace(const char* what);
    void reset_lane();
    struct HostRun;  // a host run and its threads (batch_host.hip; DESIGN.md, "Host buffers in, host hits out")
    void host_room(uint64_t n, uint64_t total_bases, bool trace);
    void finish_lane();
    void size_hit_workspace(uint64_t cap);  // the ten seed-hit arrays at `cap` entries, contents not kept
    void grow_hit_workspace(uint64_t need);
    void run_range(const mtsv_params& p, const uint8_t* raw, uint8_t* sb, const uint32_t* so, const uint32_t* h_off, uint64_t n,
                   uint32_t range_max_len, uint64_t read_base);
    void run_slice(const mtsv_params& p, const uint8_t* sb, const uint32_t* so, const uint32_t* h_off, uint64_t n_slice,
                   uint32_t slice_max_len, uint64_t read_base);
    void end_run();
    // A pass of run_slice and its stages (batch_pass.hip; DESIGN.md, "How a pass is laid out")
    struct Pass;
    struct Round;
    enum class Seeded { kGoOn, kSameReads, kHalfReads };  // what the seed stage found: go on, or the pass again
    void room_seed_slots(const PassPlan& pl);
    void room_planes(const PassPlan& pl);
    void room_strip(uint64_t need);
    void room_hits(uint64_t total_out);
    Seeded stage_seeds(Pass& ps);
    void stage_locate(Pass& ps);
    void stage_candidates(Pass& ps);
    void stage_verify(Pass& ps);
    void verify_tiled(Pass& ps, EvalArgs& a);
    void verify_rounds(Pass& ps, const EvalArgs& a);
    void round0_diag(Pass& ps, Round& r);
    void round0_bound(Pass& ps, Round& r);
    void round0_top(Pass& ps, Round& r);
    void round_tail(Pass& ps, Round& r, const EvalArgs& a);
    void round0_times();
    void stage_gather(Pass& ps);
    void stage_commit(Pass& ps);
};

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

extern int g_default_verify_mode;  // mtsv_set_default_verify_mode

// page-locked host memory for the callers' read buffers (mtsv_host_alloc & co.)
void* host_pinned_alloc(uint64_t bytes);
void host_pinned_free(void* p);
bool host_pinned_register(void* p, uint64_t bytes);
bool host_pinned_unregister(void* p);
bool host_pinned(const void* p, uint64_t bytes);

}  // namespace mtsv

struct mtsv_batch {
    mtsv::Batch impl;
    template <class... A>
    explicit mtsv_batch(A&&... a) : impl(std::forward<A>(a)...) {}
};
