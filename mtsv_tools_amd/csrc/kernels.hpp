// kernels.hpp -- launch interface of the hot-path kernels.
//
// The mtsv-binner hot path as gfx950 kernels (k_seed.hip, k_coalesce.hip, k_verify.hip; k_report.hip for the taxa report, k_match.hip for
// the per-read match flags, k_compact.hip for the hand-over of a run's unmatched or matched reads to another workspace,
// k_merge.hip for the per-read merge of several runs' hits, k_fold.hip for the accumulator of assignment records that a
// chunk's run is folded into before the chunk leaves the device, k_parse.hip for result text parsed back into such records).
//
// One batch of reads flows through staged kernels with worklists in HBM:
//
//   k_search    lane per (read, strand, seed): FMIndex::backward_search           index.rs:305
//   k_thin      lane per strand: adaptive seed thinning / max_hits filter         index.rs:293-344,354
//               (and, a lane pair per read: the read's bit planes for k_edit_myers, its N count)
//               (k_thin_tiled: the same by tiles of 128 reads, out of LDS -- the passes seed_tile_fits() accepts)
//   scan        exclusive scan of per-strand seed-hit counts
//   k_expand    lane per kept seed: its SA rows / text positions (Interval::occ)  index.rs:347-352
//               (k_expand_tiled, behind k_thin_tiled: offsets from the counts themselves, no seed_pre)
//   k_locate    lane per seed hit with wavefront refill: SampledSuffixArray::get  index.rs:347
//   k_coalesce  wavefront per strand: sort, coalesce_seed_sites, min_seeds, rank  index.rs:358-369,435-487
//   k_sw_pairs  16-lane group per two candidates: the SW prefilter                index.rs:401-406, ssw.c:123-328
//   k_edit_myers  lane per candidate that passed it: bit-vector edit distance     index.rs:407-410, align.rs:28-85
//               (rounds follow the same-TaxId chains of the ordered loop)
//   k_evaluate  longer reads (tiled beyond 256 bases): both in one sweep + sw_sse2_word  ssw.c:354-530
//   k_resolve   lane per strand: cut-offs and rank order of the selection loop    index.rs:384-428
//   scan + k_gather  compact per-strand hits into (read, strand, rank) order      binner.rs:128
//   k_report    (taxa report on) lane per read: per-TaxID read counts of the pass   collapse.rs:120-146
//   k_match     (match flags on) lane per read: one bit, "the read has a hit"      mtsv-partition.rs:34-54
//   k_collapse  (assignments on) per read: one (tax_id, smallest edit) per TaxID      binner.rs:355-378
//   k_fold      (mtsv_fold) two sorted record lists into one, one record per key       collapse.rs:269-297, :603-625
//   k_parse     (mtsv_fold_add_text) result text back into a sorted, reduced record list     collapse.rs:198-255
//
// All arithmetic is integer; positions are u32 (n < 2^32).  No MFMA: the path is rank queries and
// small dynamic programs.
#pragma once
#include <algorithm>

#include "dev_layout.hpp"
#include "pass_plan.hpp"

namespace mtsv {

struct DevHit {  // byte-identical to mtsv_hit (include/mtsv_amd.h)
    uint64_t read;
    uint32_t tax_id;
    uint32_t gi;
    uint32_t edit;
    uint8_t strand;
    uint8_t pad[3];
    uint64_t offset;
};
static_assert(sizeof(DevHit) == 32, "DevHit must match mtsv_hit");

// The slots of a lane's counter block (Batch::d_counters, u64 each; published to Batch::h_counters).  Per slot: width;
// writer; reader; who zeroes it.  "run" = Batch::reset_lane zeroes the whole block when a run begins and nothing else does;
// "pass" = the clear of the candidates stage (kCtrClearPass, with the rounds path kCtrClearRound0 too; MTSV_FUSED_CLEAR=0: a
// memset each); "round" = ctr_clear_round() before every verify round after the first.
enum CtrSlot : uint32_t {
    kCtrSeedHits = 0,      // u64; launch_scan over the strands' seed hits (stored, not added); host: the pass's seed hits; run
    kCtrWorklist = 1,      // lo: round-0 work list length; k_coalesce*; the verify kernels, k_sw_*.  hi: heavy strands listed;
                           //   k_coalesce; k_coalesce_heavy, host trace.  pass
    kCtrLfSteps = 2,       // u64; k_locate adds; host statistic at the run's end; run
    kCtrCandidates = 3,    // u64; k_coalesce* add; host statistic at the run's end; run
    kCtrVerified = 4,      // u64; k_coalesce*, verify kernels add; host statistic at the run's end; run
    kCtrWindowBytes = 5,   // u64; k_coalesce*, verify kernels add; host statistic at the run's end; run
    kCtrOutTotal = 6,      // u64; launch_scan over the strands' hits (stored); host: the pass's hits; run
    kCtrWlCursor = 7,      // lo: claim cursor of the one-launch paths (k_evaluate, tiled, edit-first k_edit_myers); the same; pass
    kCtrSwCursor = 8,      // lo: claim cursor of k_sw_pairs and k_sw_diag; the same; pass (round 0), round, and after the top-half sweep
    kCtrPassCount = 9,     // lo: pass list length; k_sw_pairs, k_sw_diag, bound-mode k_edit_myers; list-mode k_edit_myers, host; pass, round
    kCtrMyersCursor = 10,  // lo: claim cursor of list-mode k_edit_myers; the same; pass, round
    kCtrNext0 = 11,        // lo: work list length of the next round, written by even rounds; list-mode k_edit_myers; the next
    kCtrNext1 = 12,        //   round's kernels, host.  kCtrNext1: by odd rounds.  The slot a round writes: pass (kCtrNext0), round
    kCtrMaxWindow = 13,    // u64; k_max_window (max); host: strip length of a tiled pass; a memset before that launch
    kCtrSwCellPairs = 14,  // u64; k_sw_pairs adds; host statistic at the run's end; run
    kCtrMidStrands = 15,   // lo: strands listed for k_coalesce_mid.  hi: strands of 13..16 seed hits.  k_coalesce; the later
                           //   coalescing kernels, host trace; pass
    kCtrSweepCount = 16,   // lo: sweep list length; k_sw_diag; k_sw_pairs, bound-mode k_edit_myers; a memset before k_sw_diag
    kCtrUndecided = 17,    // lo: undecided list length; bound/fused k_edit_myers, top-half k_sw_pairs; k_sw_pairs, host
                           //   (MTSV_TAIL_FROM_LIST); pass (rounds path), else a memset before its writer
    kCtrBoundCursor = 18,  // lo: claim cursor of bound/fused k_edit_myers; the same; pass (rounds path), else with kCtrUndecided
    kCtrMyersColumns = 19, // u64 each, EvalArgs::myers_ctr[0..2]: columns advanced, candidates the bound refuted, successors the
    kCtrBoundRefuted = 20, //   list mode's bound passed; k_edit_myers adds; host statistics at the run's end; run
    kCtrListPassed = 21,
    kCtrListedSlots = 22,  // lo: seed slots listed for the general search; k_search; k_search_listed, host; pass (after the host
                           //   has read it: Batch::listed_zero), else a memset in launch_search
    kCtrHeavyWalk = 23,    // lo: strands k_coalesce_heavy walked by runs, hi: by the wavefront walk (a run too long); host trace; run
    kCtrHeavyTicket = 24,  // lo: next strand of the heavy list to claim; k_coalesce_heavy; the same; pass, else a memset in launch_coalesce
    kCtrCount
};
constexpr uint64_t ctr_bit(uint32_t slot) { return 1ull << slot; }
// what launch_clear_counters zeroes before the coalescing kernels of a pass; on the rounds path also what round 0 starts from
// (no coalescing kernel touches those); before round > 0
constexpr uint64_t kCtrClearPass = ctr_bit(kCtrWorklist) | ctr_bit(kCtrWlCursor) | ctr_bit(kCtrMidStrands) | ctr_bit(kCtrHeavyTicket) | ctr_bit(kCtrListedSlots);
constexpr uint64_t ctr_clear_round(uint32_t round) {
    return ctr_bit(kCtrSwCursor) | ctr_bit(kCtrPassCount) | ctr_bit(kCtrMyersCursor) | ctr_bit(kCtrNext0 + (round & 1));
}
constexpr uint64_t kCtrClearRound0 = ctr_clear_round(0) | ctr_bit(kCtrUndecided) | ctr_bit(kCtrBoundCursor);
static_assert(kCtrCount <= 64, "launch_clear_counters takes a mask of 64 slots");
static_assert(kCtrNext1 == kCtrNext0 + 1, "the rounds ping-pong between two adjacent slots");
static_assert(kCtrPassCount == kCtrSwCursor + 1 && kCtrMyersCursor == kCtrSwCursor + 2, "one memset zeroes the three of a round");
static_assert(kCtrBoundCursor == kCtrUndecided + 1, "one memset zeroes the bound pass's two");
static_assert(kCtrBoundRefuted == kCtrMyersColumns + 1 && kCtrListPassed == kCtrMyersColumns + 2, "EvalArgs::myers_ctr is an array of three");
static_assert(kCtrVerified == kCtrCandidates + 1 && kCtrWindowBytes == kCtrCandidates + 2, "k_coalesce adds to the three side by side");

struct EvalArgs {
    const uint8_t* bases;
    const uint32_t* read_off;
    uint32_t r0;
    double edit_rate;
    int64_t max_candidates;
    const uint32_t* strand_off;
    const uint4* cand;            // (start, end, bin, strand) in rank order per strand
    const uint32_t* cand_next;    // rank of the next candidate with the same TaxId, 0xffffffff = none
    uint32_t* cand_status;        // 0 not verified, 1 failed, 2 passed
    const uint32_t* worklist;     // candidate indices of this round
    const uint32_t* wl_count;
    uint32_t* wl_cursor;         // dynamic scheduling: next unclaimed worklist position
    uint32_t wl_reverse = 0;     // k_sw_pairs, k_edit_myers in fused mode: consume the worklist from its end
    // k_sw_pairs: the lane's counter block (kCtr* slots below) and the slot whose low word holds its worklist length
    uint64_t* counters = nullptr;
    uint32_t wl_count_slot = 0;
    uint4* out;                   // out[candidate] = (tax_id, gi, offset, edit) when it passed
    unsigned long long* n_verified;
    unsigned long long* window_bytes;
    unsigned long long* sw_columns = nullptr;  // k_sw_pairs: packed DP cell pairs swept (group columns x rows per lane)
    // reference order, reads <= 253 bases: k_sw_pairs appends candidates that pass the prefilter to
    // pass_list; k_edit_myers (list mode) verifies them and appends the successors of those that fail
    // the edit distance to next_list, the worklist of the next round
    uint32_t* pass_list = nullptr;
    uint32_t* pass_count = nullptr;
    uint32_t* next_list = nullptr;
    uint32_t* next_count = nullptr;
    unsigned long long* myers_ctr = nullptr;  // k_edit_myers: [0] += columns its recurrences advanced, [1] += candidates its bound refuted,
                                              // [2] += successors the list mode's own bound passed (they count as sent on to the edit distance)
    uint32_t* und_list = nullptr;  // k_sw_pairs TOP / k_edit_myers bound mode: candidates they do not decide
    uint32_t und_slot = 0;
    // tiled long-read kernel: one strip of strip_len window columns per 16-lane group (bottom row of a band)
    uint2* strip = nullptr;
    uint32_t strip_len = 0;
    // k_edit_myers: the bit planes of the pass's reads, written by k_thin for every read with a seed hit on either strand
    // (only those have work items; the others' entries are never written nor read).  Read i of the pass (i = strand index
    // >> 1) owns 3 * plane_words words at planes[3 * plane_words * i]: word j of its planes at [3j] (bit 0 of the code),
    // [3j + 1] (bit 1) and [3j + 2] (is N, code >= 4), base q of the forward read being bit q & 31 of word q >> 5.  Bits past
    // the read's end are 0; words past its last are not written.  plane_words = myers_words(longest read of the pass).
    const uint32_t* planes = nullptr;
    uint32_t plane_words = 0;
    // filled in by the launchers
    uint32_t maxc = 0xffffffffu;  // max_candidates as a bound on candidate ranks
    uint32_t claim_shift = 0;     // k_sw_pairs: work items per claim = clamp(n_work >> claim_shift, 4, 32)
};

// (myers_words(), kMaxRegisterReadLen and kMaxReadLen: pass_plan.hpp)

// n <= 64 counters from HBM into mapped page-locked host memory, by a kernel on stream s (no copy engine involved)
void launch_publish(hipStream_t s, const uint64_t* src, uint64_t* dst_host, uint32_t n);
// zeroes counters[i] for every bit i < 64 set in mask: the counters a stage starts from, in one launch
void launch_clear_counters(hipStream_t s, uint64_t* counters, uint64_t mask);
// base normalisation of bytes [begin, end) of a read buffer, src -> dst (may be equal): every other kernel expects codes
void launch_normalise(hipStream_t s, const uint8_t* src, uint8_t* dst, uint64_t begin, uint64_t end);
// run_host's transfer format (4-bit codes, host_pack.hpp) into byte codes: bytes [lo, hi) of dst from packed[lo / 2 ...]
void launch_unpack(hipStream_t s, const uint8_t* packed, uint8_t* dst, uint64_t lo, uint64_t hi);
void launch_search(hipStream_t s, const DevIndexView& ix, const uint8_t* bases, const uint32_t* read_off, uint32_t r0,
                   uint32_t n_reads, uint32_t max_ns, uint32_t K, uint32_t G, uint32_t* seed_lo, uint32_t* seed_cnt,
                   uint32_t* slow_list, uint32_t* slow_count, uint32_t listed_cap, const uint2* kmer_levels,
                   bool count_is_zero = false);
// count_is_zero: the caller has zeroed *slow_count on this stream already (launch_clear_counters)
// slow_list: room for every seed slot; *slow_count: a counter of the lane; listed_cap: list entries the second kernel's grid covers
// (the caller compares *slow_count with it afterwards); kmer_levels: DeviceIndex::d_kmer_levels, or null (a kernel argument of
// its own: the index view is at k_search_fast's scalar-register budget as it is)
// strand_nseeds receives one word per strand for the coalescing kernels: min_seeds (index.rs:358) | edit tolerance << 16 |
// a flag for the strands no candidate of which can be accepted (more N in the read than the edit tolerance, or the usize
// wrap of index.rs:406).  planes (may be null: a pass k_edit_myers does not verify): the bit planes of EvalArgs::planes,
// plane_words words per plane and read
void launch_thin(hipStream_t s, const uint8_t* bases, const uint32_t* read_off, uint32_t r0, uint32_t n_reads, double edit_rate,
                 double min_seed, uint32_t max_ns, uint32_t K, uint32_t G, uint64_t max_hits, uint64_t tune, uint32_t* seed_cnt, uint32_t* seed_pre,
                 uint32_t* strand_hits, uint32_t* strand_nseeds, uint32_t* planes, uint32_t plane_words);
// The seed stage by tiles (k_thin_tiled, k_expand_tiled): the same outputs without seed_pre -- k_expand_tiled forms a kept
// seed's offset from the counts k_thin_tiled left.  For the passes seed_tile_fits() accepts (max_ns <= seed_tile_max_ns(),
// reads up to kMaxRegisterReadLen bases, fewer than 2^32 slots); the two launches of a pass go together, tiled or not.
bool seed_tile_fits(uint32_t max_ns, uint32_t max_len, uint64_t n_slots);
uint32_t seed_tile_reads();   // reads per workgroup of k_thin_tiled
uint32_t seed_tile_max_ns();
void launch_thin_tiled(hipStream_t s, const uint8_t* bases, const uint32_t* read_off, uint32_t r0, uint32_t n_reads, double edit_rate,
                       double min_seed, uint32_t max_ns, uint32_t K, uint32_t G, uint64_t max_hits, uint64_t tune, uint32_t* seed_cnt,
                       uint32_t* strand_hits, uint32_t* strand_nseeds, uint32_t* planes, uint32_t plane_words);
void launch_expand_tiled(hipStream_t s, const DevIndexView& ix, uint32_t n_strands, uint32_t max_ns, uint32_t G, const uint32_t* seed_lo,
                         const uint32_t* seed_cnt, const uint32_t* strand_off, uint32_t* hit_row, uint32_t* hit_ref, uint32_t* hit_q);
// out has n+1 entries (out[n] = total); tile_sums needs scan_tiles(n) entries
void launch_scan(hipStream_t s, const uint32_t* in, uint32_t n, uint64_t* tile_sums, uint64_t* total, uint32_t* out);
uint32_t scan_tiles(uint32_t n);
void launch_expand(hipStream_t s, const DevIndexView& ix, uint32_t n_strands, uint32_t max_ns, uint32_t G,
                   const uint32_t* seed_lo, const uint32_t* seed_cnt, const uint32_t* seed_pre, const uint32_t* strand_off,
                   uint32_t* hit_row, uint32_t* hit_ref, uint32_t* hit_q);
void launch_locate(hipStream_t s, const DevIndexView& ix, uint32_t total_hits_host, const uint32_t* total_hits_dev,
                   const uint32_t* hit_row, uint32_t* hit_ref, unsigned long long* lf_steps);
void launch_coalesce(hipStream_t s, const DevIndexView& ix, const uint32_t* read_off, uint32_t r0, uint32_t n_strands,
                     int64_t max_candidates, const uint32_t* strand_off,
                     const uint32_t* strand_nseeds, const uint32_t* hit_ref, const uint32_t* hit_q, uint64_t* hit_key,
                     uint64_t* cand_tmp, uint4* cand, uint32_t* cand_next, uint32_t* cand_status,
                     uint32_t* strand_ncand, uint32_t* worklist, uint32_t* heavy_list, uint64_t* counters,
                     bool ticket_is_zero = false);
// ticket_is_zero: the caller has zeroed counters[kCtrHeavyTicket] on this stream already (launch_clear_counters)
void launch_evaluate(hipStream_t s, const DevIndexView& ix, const EvalArgs& a, uint64_t max_items, uint32_t max_len);
// reads of kMaxRegisterReadLen + 1 .. kMaxReadLen bases: the same sweep in bands of 256 rows (a.strip / a.strip_len set:
// tiled_groups(max_items, strip_len) strips of strip_len uint2 each, strip_len >= the pass's longest window)
void launch_evaluate_tiled(hipStream_t s, const DevIndexView& ix, const EvalArgs& a, uint64_t max_items);
uint32_t tiled_groups(uint64_t max_items, uint32_t strip_len);
void launch_max_window(hipStream_t s, uint32_t n_strands, const uint32_t* strand_off, const uint32_t* strand_ncand,
                       const uint4* cand, unsigned long long* out);
// Myers bit-vector edit distance, lane per candidate (reads up to 253 bases).
// mode 0: edit-first order over the same-TaxId chains; 1: the candidates of a.worklist that passed the SW prefilter
// (reference order); 2: the recurrence as a two-sided bound on the prefilter's predicate itself -- what it proves to
// pass goes to a.pass_list, what it refutes is marked failed (and the TaxId's next candidate bounded), the rest goes
// to a.und_list (count in the low word of counter slot a.und_slot), flagged, for launch_sw_pairs; a.counters set
// 3: fused -- bound and edit distance of the unfiltered worklist (read from its end when a.wl_reverse) in one pass: refutes
// as mode 2 does, accepts into a.out what the bound passes when read or window holds no N (a second pass under the edit
// distance's matches otherwise), and leaves the rest on a.und_list like mode 2; a.pass_list is not written
// wgs_per_cu: the grid is capped at 256 * wgs_per_cu persistent workgroups of 30 KiB of LDS each (1..5; five fill a CU's
// LDS, fewer leave room for other streams' kernels beside them).  listed: max_items counts the entries of the work list
// itself (known on the host), not the pass's seed hits: a lane per entry.  legacy_fetch: every lane fetches its own window, two
// 16-byte pieces per 16 columns (fetch_cols), instead of the quads fetching whole sectors
constexpr uint32_t kMyersWgsPerCuMax = 5;
// returns the grid it launched, in workgroups
uint32_t launch_edit_myers(hipStream_t s, const DevIndexView& ix, const EvalArgs& a, uint64_t max_items, uint32_t max_len,
                           int mode = 0, uint32_t wgs_per_cu = kMyersWgsPerCuMax, bool listed = false, bool legacy_fetch = false);
// reference order for reads <= 253 bases: SW prefilter alone, two candidates per 16-lane group
// diag = false: without the lower bounds on the seed diagonal (every candidate that is not hopeless is swept)
// top = true: the sweep on the top half of the read rows (k_sw_pairs<R/2, false, TOP>): refutes or passes what those rows
// decide, appends the rest to a.und_list (count in the low word of counter slot a.und_slot), flagged, for a second launch
// sparse = true: the work list holds a small fraction of max_items (what the edit-distance bound left): a small grid
void launch_sw_pairs(hipStream_t s, const DevIndexView& ix, const EvalArgs& a, uint64_t max_items, uint32_t max_len,
                     bool diag = true, bool top = false, bool sparse = false);
// the prefilter's lower bounds alone, a lane per work item: decided candidates go to a.pass_list (count in kCtrPassCount),
// the others to sweep_list (count in the low word of counter slot sweep_slot), flagged, for launch_sw_pairs
void launch_sw_diag(hipStream_t s, const DevIndexView& ix, const EvalArgs& a, uint64_t max_items, uint32_t max_len,
                    uint32_t* sweep_list, uint32_t sweep_slot);
void launch_resolve(hipStream_t s, uint32_t n_strands, int64_t max_candidates, int64_t max_assignments,
                    const uint32_t* strand_off, const uint32_t* strand_ncand, const uint32_t* cand_status, uint4* out,
                    uint32_t* strand_nout);
void launch_gather(hipStream_t s, uint32_t n_strands, uint64_t r0, const uint32_t* strand_off, const uint32_t* strand_nout,
                   const uint32_t* out_off, const uint4* out, DevHit* hits, uint64_t hits_base);
// k_report.hip: the per-TaxID read counts of a pass (collapse.rs:120-146) from its gathered hits.  hits: the pass's first
// hit (read r of the pass owns strand_nout[2r] + strand_nout[2r + 1] entries from out_off[2r] on); taxa: the index's n_taxa
// distinct TaxIDs, ascending; counts: 4 u64 per taxon (only_hit, only_best, tied_best, not_best); *total_reads: reads with
// a hit.  dense: the workgroups count in 4 * n_taxa LDS counters (n_taxa <= kReportDenseTaxa), else in an LDS hash table of
// hash_slots entries (a power of two, 16 .. kReportHashSlots).  n_global (may be null; MTSV_TRACE): += the atomic adds the
// launch made on counts and total_reads
constexpr uint32_t kReportDenseTaxa = 4095;  // 4 * 4095 u32 and the read counter: 64 KiB, two workgroups per CU
constexpr uint32_t kReportHashSlots = 4096;
void launch_report(hipStream_t s, uint32_t n_reads, const uint32_t* strand_nout, const uint32_t* out_off, const DevHit* hits,
                   const uint32_t* taxa, uint32_t n_taxa, bool dense, uint32_t hash_slots, uint64_t* counts, uint64_t* total_reads,
                   uint64_t* n_global);
// k_match.hip: the match flags of a pass.  Read r of the pass (strand_nout[2r], [2r + 1]: its hits per strand) sets bit
// (first_bit + r) & 63 of words[(first_bit + r) >> 6] when it has a hit -- atomically: other streams may be writing the same
// words -- and *n_matched grows by the number of such reads.  The words must be zero where no read has been flagged yet.
void launch_match(hipStream_t s, uint32_t n_reads, const uint32_t* strand_nout, uint64_t first_bit, uint64_t* words, uint64_t* n_matched);
// k_compact.hip: the reads of a resident batch (codes, read_off[n_reads + 1]) whose bit in `words` (bit r = read r) is clear
// (keep_matched: set), in order, as the resident batch of another workspace.  The scan: tile_cnt / tile_bases
// (compact_tiles(n_reads) entries each) become the exclusive prefixes of the survivors and of their bases per tile of reads,
// result[0] = survivors m, [1] = their bases, [2] = the longest of them (the caller zeroes [2] first).  The copy, once the
// host has checked m and the bases against the destination: dst_off[0 .. m] (from 0), dst_map[j] = src_map[i] (src_map
// null: i) for survivor j = source read i, dst_codes = the survivors' codes.  codes must be readable four bytes past its
// last base; nothing is written behind dst_codes' last.
uint32_t compact_tiles(uint64_t n_reads);
void launch_compact_scan(hipStream_t s, uint32_t n_reads, const uint64_t* words, const uint32_t* read_off, int keep_matched, uint64_t* tile_cnt,
                         uint64_t* tile_bases, uint64_t* result);
void launch_compact_copy(hipStream_t s, uint32_t n_reads, const uint64_t* words, const uint32_t* read_off, const uint8_t* codes, int keep_matched,
                         const uint32_t* src_map, const uint64_t* tile_cnt, const uint64_t* tile_bases, const uint64_t* result, uint8_t* dst_codes,
                         uint32_t* dst_off, uint32_t* dst_map);
// hits[i].read = map[hits[i].read] for the n_hits hits a pass of a compacted workspace has just gathered
void launch_remap_reads(hipStream_t s, DevHit* hits, uint64_t n_hits, const uint32_t* map);
// k_merge.hip: the hits of several runs over the same n_reads resident reads, merged per read in source order.  A PART is a
// stretch of one source's hits: `count` hits ordered by `read`, all the hits that source has for resident reads
// [first_read, first_read + n_reads); the parts of a source cover every read once.  map (null: the identity): resident read
// -> the number its hits carry, ascending.  Without a map the key of resident read j is j itself: that rests on a resident
// mtsv_batch_run numbering its hits from 0.  A resident run with a read base of its own would need the base in the part;
// as it stands every hit of such a run would count as dropped, which merge_runs reports as an internal error.
// Arrays per (source, read) are indexed [src * n_reads + read].
//   bounds: lo = the read's first hit in its part, cnt = how many it has there
//   sum:    nout[2j] = read j's merged count, nout[2j + 1] = 0; cnt_base: counts in, the copy's offsets out
//   (launch_scan over the 2 * n_reads entries of nout: out_off)
//   copy:   every hit of every part to its place among dst[0 .. n_dst); *n_dropped (zeroed by the caller) += the hits
//           that have no read in their part or no place in dst -- none, unless a part is not ordered as stated
// max_part_reads / max_part_hits: the largest n_reads / count of any part (the grids' x extent; n_parts is their y: < 65536)
struct MergePart {
    const DevHit* hits;
    uint32_t count, first_read, n_reads, src;
    uint64_t pad;
};
static_assert(sizeof(MergePart) == 32, "MergePart is uploaded as it is");
void launch_merge_bounds(hipStream_t s, const MergePart* parts, uint32_t n_parts, uint32_t max_part_reads, uint32_t n_reads,
                         const uint32_t* map, uint32_t* lo, uint32_t* cnt);
void launch_merge_sum(hipStream_t s, uint32_t n_reads, uint32_t n_srcs, const uint32_t* lo, uint32_t* cnt_base, uint32_t* nout);
void launch_merge_copy(hipStream_t s, const MergePart* parts, uint32_t n_parts, uint32_t max_part_hits, uint32_t n_reads,
                       const uint32_t* map, const uint32_t* base, const uint32_t* out_off, DevHit* dst, uint32_t n_dst, uint64_t* n_dropped);
// k_collapse.hip: the assignments of a pass (binner.rs:355-378) from its gathered hits -- per read one record (read, tax_id,
// smallest edit) per distinct TaxID, ascending by TaxID as unsigned, reads in the order of the hits.  Inputs as for
// launch_report; n_hits: the pass's hits (known on the host).  keys (n_hits u64), flags and place (n_hits + 1 u32 each),
// tile_sums (scan_tiles(n_hits) + 1) and list (n_reads u32) are scratch; ctr: kCollapseCounters u64, zeroed here, of which
// [kCollapseCtrTotal] receives the number of records written to out[0 ..) (at most n_hits; byte-identical to
// mtsv_assignment) and [kCollapseCtrLane ..] the reads every tier took.  Tiers by a read's hit count: up to lane_max
// (1 .. kCollapseLaneMax) a lane, up to wave_max (<= 64) its wavefront, up to lds_max (a power of two <= kCollapseLdsKeys) a
// workgroup sorting in LDS, beyond that a workgroup sorting in `keys` itself.
// grain (the values of MTSV_GRAIN_*): kCollapseGrainTaxid is the above.  The wide grains keep GI and offset: per read one
// 24-byte record (mtsv_assignment_gi) per distinct (tax_id, gi, offset) with the smallest edit, ascending by the triple
// (kCollapseGrainLong, binner.rs:320-352), or per distinct (tax_id, gi) with the smallest (edit, offset), ascending by the pair
// (kCollapseGrainTaxidGi, collapse.rs:603-625).  Their keys are 16 bytes (keys: n_hits of those, 16-byte aligned) and their
// lds_max ends at kCollapseLdsKeysWide.
constexpr uint32_t kCollapseLaneMax = 16, kCollapseLdsKeys = 4096, kCollapseLdsKeysWide = 2048;
constexpr int kCollapseGrainTaxid = 0, kCollapseGrainTaxidGi = 1, kCollapseGrainLong = 2;
constexpr uint32_t kCollapseCtrTotal = 0, kCollapseCtrList = 1, kCollapseCtrTicket = 2, kCollapseCtrLane = 3, kCollapseCtrWave = 4,
                   kCollapseCtrListed = 5, kCollapseCtrLds = 6, kCollapseCtrGlobal = 7, kCollapseCounters = 8;
void launch_collapse(hipStream_t s, int grain, uint32_t n_reads, const uint32_t* strand_nout, const uint32_t* out_off, const DevHit* hits,
                     uint32_t n_hits, uint32_t lane_max, uint32_t wave_max, uint32_t lds_max, void* keys, uint32_t* flags, uint32_t* place,
                     uint64_t* tile_sums, uint32_t* list, uint64_t* ctr, void* out);
// k_fold.hip: two assignment lists of one grain (records as launch_collapse writes them, each list ascending by the grain's
// key -- (read, tax_id), (read, tax_id, gi, offset) or (read, tax_id, gi), unsigned -- with distinct keys) folded into their
// sorted union, one record per key: for a key both lists hold, a's record with the smaller edit of the two (TAXID_GI: the
// smaller (edit, offset)).  a and b are 16-byte aligned, n_a + n_b < 2^32.  A workgroup owns `tile` positions (a power of two,
// 2 .. kFoldTileMax) of the merged sequence; there are fold_tiles(n_a + n_b, tile) of them.
//   count:  tile_cnt[t] = the records tile t keeps
//   (launch_scan over tile_cnt: tile_off[0 .. tiles], tile_off[tiles] = the records of the union)
//   write:  the union to out[0 .. tile_off[tiles]); a tile writes nothing outside [tile_off[t], tile_off[t + 1])
constexpr uint32_t kFoldTileMax = 1024, kFoldTile = 1024;
uint32_t fold_tiles(uint64_t n, uint32_t tile);
void launch_fold_count(hipStream_t s, int grain, const void* a, uint32_t n_a, const void* b, uint32_t n_b, uint32_t tile, uint32_t* tile_cnt);
void launch_fold_write(hipStream_t s, int grain, const void* a, uint32_t n_a, const void* b, uint32_t n_b, uint32_t tile, const uint32_t* tile_off,
                       void* out);
// The match flags of a list: every read that has a record sets bit (read & 63) of words[read >> 6] (zeroed by the caller) and
// adds one to ctr[0]; a read >= n_reads sets nothing and adds one to ctr[1].  ctr: two u64, zeroed by the caller.
void launch_fold_flags(hipStream_t s, int grain, const void* rec, uint32_t n, uint64_t n_reads, uint64_t* words, uint64_t* ctr);
// The taxa report of a list (launch_report's categories, from per read {tax_id -> smallest edit of its records}): counts holds
// 4 u64 per taxon of the ascending list taxa, then the reads with a record, then the (read, TaxID) pairs whose TaxID the list does
// not hold (they are counted nowhere else); 4 * n_taxa + 2 u64, zeroed by the caller.
void launch_fold_report(hipStream_t s, int grain, const void* rec, uint32_t n, const uint32_t* taxa, uint32_t n_taxa, uint64_t* counts);
// k_text.hip: the result lines of n assignment records of one grain (ordered by the grain's key, 4-byte aligned), as
// mtsv_format_assignments / _gi write them.  ids (4-byte aligned, ids_bytes of them) and id_off[n_reads + 1] are the read
// IDs on the device; a workgroup owns `tile` records (a power of two, 2 .. kTextTileMax); there are text_tiles(n, tile) tiles.
//   measure: rec_len[i] = the bytes of record i, tile_cnt[t] = the bytes of tile t; ctr[0] += the reads at or above n_reads,
//            ctr[1] += the ID slots outside the ID bytes or longer than kTextIdMax (ctr: two u64, zeroed by the caller)
//   scan:    tile_off[0 .. tiles] = the byte at which a tile's text begins, tile_off[tiles] = *total = the bytes of the text;
//            sums: text_scan_blocks(tiles) u64 of scratch
//   write:   the text to out[0 .. total); a tile writes nothing outside [tile_off[t], tile_off[t + 1]).  Only after a
//            measure pass that left both counters at zero.
constexpr uint32_t kTextTileMax = 1024, kTextTile = 1024;
constexpr uint64_t kTextIdMax = 1ull << 20;
uint32_t text_tiles(uint64_t n, uint32_t tile);
uint32_t text_scan_blocks(uint32_t tiles);
uint32_t text_window_bytes(uint32_t tile);  // the LDS image of a tile: longer texts leave in several windows
void launch_text_measure(hipStream_t s, int grain, const void* rec, uint32_t n, const uint8_t* ids, const uint64_t* id_off, uint64_t n_reads,
                         uint64_t ids_bytes, uint32_t tile, uint32_t* rec_len, uint32_t* tile_cnt, uint64_t* ctr);
void launch_text_scan(hipStream_t s, const uint32_t* tile_cnt, uint32_t tiles, uint64_t* sums, uint64_t* total, uint64_t* tile_off);
void launch_text_write(hipStream_t s, int grain, const void* rec, uint32_t n, const uint8_t* ids, const uint64_t* id_off, uint32_t tile,
                       const uint32_t* rec_len, const uint64_t* tile_off, uint8_t* out);
// k_pack.hip: the file's raw bytes into the HBM layout, for upload_index under MTSV_DEV_PACK_ON_DEVICE.  bwt: n raw bytes;
// blocks: n_blocks = (n >> 7) + 1 rank blocks; a workgroup owns `tile` blocks (a power of two, 1 .. kPackTileMax); there are
// pack_tiles(n_blocks, tile) tiles.  ctr: kPackCounters u32, set by the caller to 0 except the two *First/*Row minima
// (0xffffffff).
//   count:  tile_cnt[t] = the A, C, G, T of tile t; ctr[kPackCtrForeign] += bytes outside ACGTN$ ([kPackCtrForeignRow]: the
//           first such row), ctr[kPackCtrSentinels] += sentinels ([kPackCtrSentinelRow]: the last one's row)
//   scan:   tile_cnt to its exclusive prefixes, in place
//   blocks: every block of every tile, byte for byte what the host packs; rows at and beyond n hold code 7
//   check_occ: occ holds the file's six Occ arrays of A C G T N $, n_chk = (n - 1) / k + 1 entries each, one after the other;
//           ctr[kPackCtrOccBad] += checkpoints that disagree with the blocks, [kPackCtrOccBadFirst] = the smallest of them.
//           Reads the sentinel counters: after count, on the same stream.
//   text:   codes[0 .. codes_bytes) (a multiple of 16) from text[0 .. n), 7 behind n; text is readable up to the next
//           multiple of 16 bytes
constexpr uint32_t kPackTileMax = 64, kPackTile = 64;
constexpr uint32_t kPackCtrForeign = 0, kPackCtrForeignRow = 1, kPackCtrSentinels = 2, kPackCtrSentinelRow = 3, kPackCtrOccBad = 4,
                   kPackCtrOccBadFirst = 5, kPackCounters = 8;
uint32_t pack_tiles(uint32_t n_blocks, uint32_t tile);
void launch_pack_count(hipStream_t s, const uint8_t* bwt, uint32_t n, uint32_t n_blocks, uint32_t tile, uint4* tile_cnt, uint32_t* ctr);
void launch_pack_scan(hipStream_t s, uint4* tile_cnt, uint32_t n_tiles);
void launch_pack_blocks(hipStream_t s, const uint8_t* bwt, uint32_t n, uint32_t n_blocks, uint32_t tile, const uint4* tile_off, RankBlock* blocks);
void launch_pack_check_occ(hipStream_t s, const RankBlock* blocks, uint32_t n, uint32_t k, uint32_t n_chk, const uint64_t* occ, uint32_t* ctr);
void launch_pack_text(hipStream_t s, const uint8_t* text, uint32_t n, uint8_t* codes, uint64_t codes_bytes);
// k_parse.hip: the hit parts of result lines (hits[0 .. n_bytes), 16-byte aligned; line j = hits[line_off[j] .. line_off[j + 1]),
// line_off[0] = 0 and ascending -- the caller has checked -- line_off[n_lines] = n_bytes; line_read[j] the line's read) into a
// list of assignment records of one grain, ordered by the grain's key with distinct keys.  A workgroup owns `tile` bytes (a
// power of two, 64 .. kParseTileMax); there are parse_tiles(n_bytes, tile) tiles.
//   count:   tile_cnt[t] = the tokens that start in tile t
//   (launch_scan over tile_cnt: tile_off[0 .. tiles], tile_off[tiles] = n_tok, which must be below 2^32)
//   tokens:  raw_key[i] (read, tax, gi, offset), raw_val[i] (edit, first of its line, line as two words): n_tok uint4 each.
//            ctr: kParseCounters u64 as pairs (how many, the smallest line), set by the caller to (0, all ones);
//            [kParseCtrFormat] the tokens outside the grammar or, in a wide grain, without GI and offset
//   heads:   flag[i] = token i begins a record; [kParseCtrKeyOrder] keys that descend inside a line, [kParseCtrReadOrder]
//            lines whose read is not above the previous non-empty line's, [kParseCtrReadRange] reads at or above n_reads
//   (launch_scan over flag: place[0 .. n_tok], place[n_tok] = n_rec)
//   reduce:  out[0 .. n_rec): the records (mtsv_assignment / mtsv_assignment_gi), every one with the smallest edit of its
//            run -- kCollapseGrainTaxidGi: the smallest (edit, offset); tax_out[0 .. n_rec): their TaxIDs.  Only after counters
//            that are all zero.
constexpr uint32_t kParseTileMax = 16384, kParseTile = 4096;
constexpr uint32_t kParseCtrFormat = 0, kParseCtrKeyOrder = 2, kParseCtrReadOrder = 4, kParseCtrReadRange = 6, kParseCounters = 8;
uint32_t parse_tiles(uint64_t n_bytes, uint32_t tile);
void launch_parse_count(hipStream_t s, const uint8_t* hits, uint64_t n_bytes, const uint64_t* line_off, uint64_t n_lines, uint32_t tile,
                        uint32_t* tile_cnt);
void launch_parse_tokens(hipStream_t s, int grain, const uint8_t* hits, uint64_t n_bytes, const uint64_t* line_off, const uint32_t* line_read,
                         uint64_t n_lines, uint32_t tile, const uint32_t* tile_off, uint32_t n_tok, void* raw_key, void* raw_val, uint64_t* ctr);
void launch_parse_heads(hipStream_t s, int grain, const void* raw_key, const void* raw_val, uint32_t n_tok, uint64_t n_reads, uint32_t* flag,
                        uint64_t* ctr);
void launch_parse_reduce(hipStream_t s, int grain, const void* raw_key, const void* raw_val, const uint32_t* flag, const uint32_t* place,
                         uint32_t n_tok, uint32_t n_rec, void* out, uint32_t* tax_out);

// k_lca.hip: per read of a sorted assignment list (n records of 4 or 6 words: read in words 0 and 1, tax_id in word 2, edit in
// the last) the lowest common ancestor of the TaxIDs whose edit is within `slack` of the read's smallest, on a tree numbered in
// preorder: node 0 is the super-root, parent[i] < i for i > 0, last[i] is the last node of i's subtree, tax[i] its TaxID;
// u_tax[0 .. n_union) ascending with u_node beside it maps a record's TaxID to its node.  A workgroup owns `tile` records (a power
// of two, 64 .. kLcaTileMax); there are lca_tiles(n, tile) tiles.  A HEAD is a record whose read differs from its predecessor's;
// the reads with a record are numbered by their heads (slots).  ctr: kLcaCounters u64, zeroed by the caller.
//   heads:  tile_cnt[t] = the heads of tile t
//   (launch_scan over tile_cnt: tile_off[0 .. tiles], tile_off[tiles] = n_slots)
//   min:    m[slot] = the smallest edit of the read (m set to all ones by the caller); out[slot].read (16-byte records)
//   span:   lo[slot] / hi[slot] = the smallest / largest node number among the records with edit <= m[slot] + slack, saturating
//           (lo set to all ones, hi to zero by the caller); ctr[kLcaCtrMissing] += records whose TaxID u_tax does not hold
//   walk:   out[slot] = (read, tax of the LCA, m[slot]); direct[node] += 1 (direct: n_nodes u32, zeroed by the caller); a walk
//           of more than max_depth steps, or a span outside the tree, adds to ctr[kLcaCtrWalk] and writes nothing
//   (launch_scan over direct: prefix[0 .. n_nodes])
//   clade:  clade[i] = prefix[last[i] + 1] - prefix[i]
constexpr uint32_t kLcaTileMax = 1024, kLcaTile = 1024;
constexpr uint32_t kLcaCtrMissing = 0, kLcaCtrWalk = 1, kLcaCounters = 2;
uint32_t lca_tiles(uint64_t n, uint32_t tile);
void launch_lca_heads(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, uint32_t* tile_cnt);
void launch_lca_min(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, const uint32_t* tile_off, uint32_t n_slots, uint32_t* m,
                    void* out);
void launch_lca_span(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, const uint32_t* tile_off, uint32_t n_slots,
                     const uint32_t* m, uint32_t slack, const uint32_t* u_tax, const uint32_t* u_node, uint32_t n_union, uint32_t* lo, uint32_t* hi,
                     uint64_t* ctr);
void launch_lca_walk(hipStream_t s, uint32_t n_slots, uint32_t n_nodes, uint32_t max_depth, const uint32_t* lo, const uint32_t* hi, const uint32_t* m,
                     const uint32_t* parent, const uint32_t* last, const uint32_t* tax, void* out, uint32_t* direct, uint64_t* ctr);
void launch_lca_clade(hipStream_t s, uint32_t n_nodes, const uint32_t* last, const uint32_t* prefix, uint32_t* clade);
// k_abund.hip: abundance by expectation-maximisation over a sorted assignment list (the definition: include/mtsv_amd.h).  Two
// kinds of heads over the n records: a READ head (the read differs from the predecessor's; the reads with a record are numbered
// by them, n_reads of them) and a RUN head (read or tax_id differs; a run is the records of one (read, tax_id), n_runs of them,
// in key order, so the runs of a read are consecutive and ascend by tax_id).  A workgroup owns `tile` records (a power of two,
// 64 .. kAbundTileMax).  ctr: kAbundCounters u64, zeroed by the caller.
//   heads:  cnt_r[t] / cnt_p[t] = the read heads / run heads of tile t
//   (launch_scan over each: off_r / off_p[0 .. tiles])
//   min:    m[read] = the read's smallest edit, e_run[run] = the run's (both set to all ones by the caller); read_id[read];
//           read_first[read] = its first run; run_tax[run], run_read[run]
//   flag:   flag[run] = e_run - m[run_read] <= slack
//   (launch_scan over flag: off[0 .. n_runs], off[n_runs] = the entries; the flagged runs of a read are its entries, consecutive)
//   write:  read_off[0 .. n_reads]; per entry its place in the union u_tax (ent_slot), min(d, n_w) (ent_d) and e_run (ent_e);
//           any[slot] += 1 per entry, uniq[slot] += 1 for the entry of a read with one (both zeroed by the caller); the reads of
//           more than lane_max entries to list[ctr[kAbundCtrList]++]; ctr[kAbundCtrMissing] += entries whose TaxID u_tax does
//           not hold, ctr[kAbundCtrLong] += reads of 65536 entries or more
//   init:   mass[slot] = any[slot] ? start : 0, next[slot] = 0
//   step:   one iteration: next[slot] += q per entry; dense: through per-workgroup counters in LDS (n_union <= kAbundDenseMax)
//   delta:  *l1 (zeroed by the caller) += |next - mass|; mass = next; next = 0
//   final:  out[read] = (read_id, tax of the entry with the largest x -- ties: the first --, its e) (16-byte records);
//           assigned[slot] += 1 (zeroed by the caller)
// w: the weight table, n_w entries.  `blocks`: the workgroups of the persistent kernels.
constexpr uint32_t kAbundTileMax = 1024, kAbundTile = 1024, kAbundLaneMax = 16, kAbundLaneMaxMax = 1024, kAbundDenseMax = 8192;
constexpr uint32_t kAbundEntriesMax = 65536;  // a read may have fewer than this many
constexpr uint32_t kAbundCtrMissing = 0, kAbundCtrLong = 1, kAbundCtrList = 2, kAbundCounters = 3;
struct AbundEntries {  // what an iteration reads
    uint32_t n_reads, n_list, lane_max, n_union;
    const uint32_t *read_off, *ent_slot, *list, *w;
    const uint8_t* ent_d;
};
uint32_t abund_tiles(uint64_t n, uint32_t tile);
void launch_abund_heads(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, uint32_t* cnt_r, uint32_t* cnt_p);
void launch_abund_min(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, const uint32_t* off_r, const uint32_t* off_p,
                      uint32_t n_reads, uint32_t n_runs, uint32_t* m, uint32_t* e_run, uint64_t* read_id, uint32_t* read_first, uint32_t* run_tax,
                      uint32_t* run_read);
void launch_abund_flag(hipStream_t s, uint32_t n_runs, const uint32_t* e_run, const uint32_t* m, const uint32_t* run_read, uint32_t slack,
                       uint32_t* flag);
void launch_abund_write(hipStream_t s, uint32_t n_reads, uint32_t n_runs, const uint32_t* off, const uint32_t* e_run, const uint32_t* m,
                        const uint32_t* run_tax, const uint32_t* run_read, const uint32_t* read_first, const uint32_t* u_tax, uint32_t n_union,
                        uint32_t n_w, uint32_t lane_max, uint32_t* read_off, uint32_t* ent_slot, uint8_t* ent_d, uint32_t* ent_e, uint32_t* any,
                        uint32_t* uniq, uint32_t* list, uint64_t* ctr);
void launch_abund_init(hipStream_t s, uint32_t n_union, const uint32_t* any, uint64_t start, uint64_t* mass, uint64_t* next);
void launch_abund_step(hipStream_t s, uint32_t blocks, bool dense, const AbundEntries& en, const uint64_t* mass, uint64_t* next);
void launch_abund_delta(hipStream_t s, uint32_t n_union, uint64_t* mass, uint64_t* next, uint64_t* l1);
void launch_abund_final(hipStream_t s, uint32_t blocks, const AbundEntries& en, const uint64_t* mass, const uint32_t* ent_e, const uint64_t* read_id,
                        const uint32_t* u_tax, void* out, uint32_t* assigned);
// k_dedup.hip: the identical reads of a resident batch (codes 0..4, read_off[n_reads + 1]; codes readable to the end of the
// aligned dword of its last base).  rep(j) = the smallest index of a read with j's length and codes.
//   hash:     hash[j], 64 bits of the read's codes and length, independent of where the read lies
//   insert:   table: n_slots u64 (a power of two >= 2 n_reads, < 2^32), set to all ones by the caller; only the low hash_bits
//             (0..64) of a hash are used; slot_of[j] = the slot of j's sequence; ctr[1] += the reads that found none (none,
//             unless the table is too small).  ctr: two u64, zeroed by the caller
//   resolve:  words: ceil(n_reads / 64) u64, bit j = "rep(j) == j"; read[j] = src_map[j], rep[j] = src_map[rep(j)] (src_map
//             null: the identity); ctr[0] += the representatives
// (launch_compact_scan / _copy with words and keep_matched = 1 then pack the representatives)
void launch_dedup_hash(hipStream_t s, uint32_t n_reads, const uint32_t* read_off, const uint8_t* codes, uint64_t* hash);
void launch_dedup_insert(hipStream_t s, uint32_t n_reads, const uint32_t* read_off, const uint8_t* codes, const uint64_t* hash, uint32_t hash_bits,
                         uint64_t* table, uint32_t n_slots, uint32_t* slot_of, uint64_t* ctr);
void launch_dedup_resolve(hipStream_t s, uint32_t n_reads, const uint64_t* table, const uint32_t* slot_of, const uint32_t* src_map, uint64_t* words,
                          uint32_t* read, uint32_t* rep, uint64_t* ctr);
// The fan: n_entries map entries (read[] strictly ascending); rec: n_rec records of the grain ordered by its key.
//   count:  first[j] / cnt[j] = where the records of read rep[j] begin in rec / how many there are; *ctr (one u64, zeroed by the
//           caller) += cnt[j] of the entries with rep[j] == read[j]
//   (launch_scan over cnt: off[0 .. n_entries], off[n_entries] = total, which must be below 2^32)
//   write:  out[off[j] .. off[j + 1]) = those records with `read` replaced by read[j].  A workgroup owns `tile` output records (a
//           power of two, 64 .. kFanTileMax)
constexpr uint32_t kFanTileMax = 1024, kFanTile = 1024;
void launch_fan_count(hipStream_t s, int grain, uint32_t n_entries, const uint32_t* read, const uint32_t* rep, const void* rec, uint32_t n_rec,
                      uint32_t* first, uint32_t* cnt, uint64_t* ctr);
void launch_fan_write(hipStream_t s, int grain, uint32_t n_entries, const uint32_t* read, const uint32_t* first, const uint32_t* off, const void* rec,
                      uint32_t tile, uint32_t total, void* out);
// k_pair.hip: the mates of read pairs joined (mode: the values of MTSV_PAIR_*).  rec: n records of the grain ordered by its key,
// reads 2p and 2p + 1 the mates of pair p, n_reads = 2P of them (below 2^32); PROPER needs kCollapseGrainLong.  A RUN is the
// records of one (read, tax_id), numbered by its head (its slot); there are at most n.  ctr: kPairCounters u64, zeroed by the
// caller.  NONE is all ones.
//   bounds: off[r] = the first record with read >= r, r in 0 .. n_reads
//   join:   val[i], and add[i] at heads (n u32 each), as the head of k_pair.hip defines them; records whose window in the other
//           mate's stretch is longer than lane_max go to list (n u32; ctr[kPairCtrList] of them); ctr[kPairCtrBadEdit] += the
//           records with edit >= 2^31, ctr[kPairCtrBeyond] += those with read >= n_reads (they join nothing)
//   wave:   the listed records' windows, a wavefront each; after join on the same stream
//   heads:  tile_cnt[t] = the heads of tile t (a power of two, 64 .. kPairTileMax; pair_tiles(n, tile) tiles)
//   (launch_scan over tile_cnt: tile_off[0 .. tiles], tile_off[tiles] = n_slots)
//   min:    m[slot] = the smallest val of the run (m: n_slots_cap u32, set to all ones by the caller), slot_rec[slot] = (read as
//           two words, tax_id, add) (n_slots_cap uint4)
//   flags:  m[slot] = the run's value m + add, or NONE when either is; flag_a[slot] = it has a value and is mate 0's,
//           flag_b[slot] (may be null) = it has one and is mate 1's; both zero from *n_slots to n_slots_cap
//   (launch_scan over flag_a and flag_b: pos_a, pos_b, n_slots_cap + 1 entries each)
//   write:  (read >> 1, tax_id, value) of the flagged slots to out_a[pos_a] / out_b[pos_b] (16-byte records; pos_b, out_b may
//           be null); nothing is written at or behind n_a / n_b
//   stats:  ctr[kPairCtrBoth] / [kPairCtrOne] += the pairs both / exactly one of whose mates have a record;
//           ctr[kPairCtrJoined] += the distinct reads of out[0 .. n_out) (16-byte records ordered by read)
constexpr int kPairBoth = 0, kPairEither = 1, kPairProper = 2;
constexpr uint32_t kPairTileMax = 1024, kPairTile = 1024, kPairLaneMax = 16, kPairLaneMaxMax = 1024;
constexpr uint32_t kPairCtrList = 0, kPairCtrBadEdit = 1, kPairCtrBeyond = 2, kPairCtrBoth = 3, kPairCtrOne = 4, kPairCtrJoined = 5, kPairCounters = 6;
uint32_t pair_tiles(uint64_t n, uint32_t tile);
void launch_pair_bounds(hipStream_t s, int grain, const void* rec, uint32_t n, uint64_t n_reads, uint32_t* off);
void launch_pair_join(hipStream_t s, int grain, int mode, const void* rec, uint32_t n, uint64_t n_reads, const uint32_t* off, uint32_t max_insert,
                      uint32_t unpaired, uint32_t lane_max, uint32_t* val, uint32_t* add, uint32_t* list, uint64_t* ctr);
void launch_pair_wave(hipStream_t s, int grain, int mode, const void* rec, uint32_t n, uint64_t n_reads, const uint32_t* off, uint32_t max_insert,
                      const uint32_t* list, const uint64_t* ctr, uint32_t* val, uint32_t* add);
void launch_pair_heads(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, uint32_t* tile_cnt);
void launch_pair_min(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, const uint32_t* tile_off, const uint32_t* val,
                     const uint32_t* add, uint32_t n_slots_cap, uint32_t* m, void* slot_rec);
void launch_pair_flags(hipStream_t s, const uint64_t* n_slots, uint32_t n_slots_cap, const void* slot_rec, uint32_t* m, uint32_t* flag_a, uint32_t* flag_b);
void launch_pair_write(hipStream_t s, const uint64_t* n_slots, uint32_t n_slots_cap, const void* slot_rec, const uint32_t* m, const uint32_t* pos_a,
                       const uint32_t* pos_b, uint32_t n_a, uint32_t n_b, void* out_a, void* out_b);
void launch_pair_stats(hipStream_t s, const uint32_t* off, uint64_t n_pairs, const void* out, uint32_t n_out, uint64_t* ctr);
// k_cover.hip: coverage per reference sequence from a list at kCollapseGrainLong (n records of 6 words ordered by (read, tax_id,
// gi, offset), n_reads below 2^32).  The table: n_refs references ascending by key = tax_id << 32 | gi, ref_len[r] bases
// each, reference r owning the words [word_off[r], word_off[r + 1]) of the bitmap (ceil(ref_len[r] / 64) of them).  A record
// COUNTS when its edit is at most m[read] + slack (saturating); a counted record (r, t, g, o, e) covers [o, min(o + read_len[r],
// L)).  A RUN is the records of one (read, tax_id, gi), numbered by its head.  NONE is all ones.  off[] comes from
// launch_pair_bounds.  ctr: kCoverCounters u64, set by the caller to 0 except [kCoverCtrFirstBad] (all ones).
//   min:    m[r] = the smallest edit of read r's records (NONE for a read without one): a lane per read walks a stretch of up
//           to kCoverMinLane records, a longer one is strided by the lanes of its wavefront
//   map:    ref[i] = the reference of record i when it counts, else NONE; head[i] = it begins a run; nothing else is written
//           but ctr: [kCoverCtrUnknown] += records whose key the table does not hold, [kCoverCtrRange] += those whose offset is
//           at or beyond their reference's length, [kCoverCtrBeyond] += those with read >= n_reads, [kCoverCtrFirstBad] = the
//           smallest i among all of these, [kCoverCtrCounted] += the records that count
//   (launch_scan over head: run[0 .. n], run[n] = the runs; record i belongs to run run[i + 1] - 1)
//   mark:   only after a map that left the first three counters at zero.  Per counted record: its interval OR-ed into the
//           bitmap by its lane when it spans up to lane_max words, else the record goes to list (n u32, ctr[kCoverCtrList] of
//           them); run_hit[its run] = 1 (zeroed by the caller), run_ref[its run] = its reference; cnt[n_refs + r] += 1 and
//           cnt[2 n_refs + r] += the interval's bases, the lanes of a wavefront that share r combined first
//   wave:   the listed records' intervals, a wavefront each; after mark on the same stream
//   reads:  cnt[r] += the runs of reference r with run_hit set (*n_runs of them, at most n)
//   pop:    cov[r] (n_refs u64, zeroed by the caller) += the bits set in reference r's words.  A workgroup owns `tile` words (a
//           power of two, 64 .. kCoverTileMax) and adds one value per reference that has words in its tile
constexpr uint32_t kCoverTileMax = 1024, kCoverTile = 1024, kCoverLaneMax = 8, kCoverLaneMaxMax = 1024, kCoverMinLane = 32;
constexpr uint32_t kCoverCtrUnknown = 0, kCoverCtrRange = 1, kCoverCtrBeyond = 2, kCoverCtrFirstBad = 3, kCoverCtrCounted = 4, kCoverCtrList = 5,
                   kCoverCounters = 6;
void launch_cover_min(hipStream_t s, const void* rec, uint32_t n, uint64_t n_reads, const uint32_t* off, uint32_t* m);
void launch_cover_map(hipStream_t s, const void* rec, uint32_t n, uint64_t n_reads, const uint32_t* m, uint32_t slack, const uint64_t* ref_key,
                      const uint32_t* ref_len, uint32_t n_refs, uint32_t* ref, uint32_t* head, uint64_t* ctr);
void launch_cover_mark(hipStream_t s, const void* rec, uint32_t n, const uint32_t* read_len, const uint32_t* ref, const uint32_t* run,
                       const uint32_t* ref_len, const uint32_t* word_off, uint32_t n_refs, uint32_t lane_max, uint64_t* bitmap, uint64_t* cnt,
                       uint32_t* run_hit, uint32_t* run_ref, uint32_t* list, uint64_t* ctr);
void launch_cover_wave(hipStream_t s, const void* rec, uint32_t n, const uint32_t* read_len, const uint32_t* ref, const uint32_t* ref_len,
                       const uint32_t* word_off, uint32_t n_refs, const uint32_t* list, const uint64_t* ctr, uint64_t* bitmap);
void launch_cover_reads(hipStream_t s, const uint64_t* n_runs, uint32_t n, const uint32_t* run_hit, const uint32_t* run_ref, uint32_t n_refs,
                        uint64_t* cnt);
void launch_cover_pop(hipStream_t s, const uint64_t* bitmap, uint32_t n_words, const uint32_t* word_off, uint32_t n_refs, uint32_t tile, uint64_t* cov);
// k_place.hip: per hit of a list (n of them, any order) the alignment's interval in its reference and its edit script, as the
// head of k_place.hip defines them.  The table: n_keys keys = tax_id << 32 | gi, strictly ascending, bin_of_key[k] the bin of
// key k among `bins`.  The reads: codes and read_off[n_reads + 1] of the resident batch; read_map (null: the identity): resident
// read -> the number its hits carry, ascending.  ctr: kPlaceCounters u64, set by the caller to 0 except the two *First* minima
// (all ones).
//   map:    hit_bin[i], hit_read[i] = the hit's bin and resident read (NONE for a hit that is refused), cnt[i] = the op slots it
//           may need, 2 min(edit, L) + 1 (0 for a refused one); nothing else is written but ctr: [kPlaceCtrUnknown] += hits whose
//           (tax_id, gi) the table does not hold, [kPlaceCtrRange] += those whose offset is at or beyond their bin's length,
//           [kPlaceCtrAbsent] += those whose read is not resident, [kPlaceCtrStrand] += those with a strand above 1,
//           [kPlaceCtrFirstBad] = the smallest i among all of these, [kPlaceCtrSpan] = the largest L + min(edit, L) of the others
//   (launch_scan over cnt: off[0 .. n], off[n] = the op slots, which must be below 2^32)
//   place:  only after a map that left the first four counters at zero.  words = myers_words(longest resident read), 2 .. 8;
//           `blocks` workgroups of place_threads() lanes stride the hits; ring: ring_cols (a power of two >= [kPlaceCtrSpan] + 2)
//           x 2 words x blocks x place_threads() u32 of scratch.  out[i] (48 bytes, mtsv_placement) and the hit's runs, in
//           reference order, at the END of ops[off[i] .. off[i + 1]): out[i].ops_off is where they begin.  A hit no column of
//           whose text reaches its edit adds to [kPlaceCtrUnplaceable] ([kPlaceCtrFirstUnplaceable]: the smallest such i) and
//           writes nothing; [kPlaceCtrBroken] += paths that left the ring or their slots (none); [kPlaceCtrColumns] += the columns
//           the placed hits stored into the ring
constexpr uint32_t kPlaceCtrUnknown = 0, kPlaceCtrRange = 1, kPlaceCtrAbsent = 2, kPlaceCtrStrand = 3, kPlaceCtrFirstBad = 4, kPlaceCtrSpan = 5,
                   kPlaceCtrUnplaceable = 6, kPlaceCtrFirstUnplaceable = 7, kPlaceCtrBroken = 8, kPlaceCtrColumns = 9, kPlaceCounters = 10;
uint32_t place_threads();
void launch_place_map(hipStream_t s, const DevHit* hits, uint32_t n, const uint64_t* bin_key, const uint32_t* bin_of_key, uint32_t n_keys, const DevBin* bins,
                      const uint32_t* read_off, uint32_t n_reads, const uint32_t* read_map, uint32_t* hit_bin, uint32_t* hit_read, uint32_t* cnt,
                      uint64_t* ctr);
void launch_place(hipStream_t s, uint32_t words, uint32_t blocks, const DevHit* hits, uint32_t n, const uint32_t* hit_bin, const uint32_t* hit_read,
                  const DevBin* bins, uint32_t n_bins, const uint8_t* text, const uint8_t* codes, const uint32_t* read_off, const uint32_t* off,
                  uint32_t* ring, uint32_t ring_cols, uint32_t* ops, void* out, uint64_t* ctr);
// k_pile.hip: the pileup of placed hits, as the head of k_pile.hip defines it.  hits, hit_bin, hit_read, out and ops are the
// placer's arrays after a placement that was not refused; bin_cnt[b]: the counters of bin b's reference ([slot][8] u32, the
// bin's length + 1 slots), or null for a bin the pileup does not select; best: n_reads u32, set by the caller to all ones.
// ctr: kPileCounters u64, zeroed by the caller.
//   best:   best[hit_read[i]] = the smallest edit among the hits of a read
//   count:  [kPileCtrSkipped] += hits in bins without counters, [kPileCtrCounted] += the others with edit <= best + slack
//           (saturating); nothing else is written
//   pile:   the counted hits' ops walked into the counters; [kPileCtrBroken] += scripts that would leave their reference (none)
//   ref:    ref[s] for the n_slots slots of a new segment of n_refs references: ref_off[n_refs + 1] their first slots
//           (ref_off[n_refs] = n_slots), text_start[r] the text position of reference r's first base; 0xff for a last slot
//   tile_sums, (launch_scan: tile_pre[pile_tiles + 1]), sites_count, (launch_scan: tile_off), sites_rows; dump: the sites of a
//           segment under (min_depth, min_alt, min_alt_ppm) as 48-byte rows in slot order, ref_key[r] = tax_id << 32 | gi; dump
//           writes slots lo .. hi - 1 as [slot - lo][8] with channel 0 integrated.  tile: a power of two, 64 .. kPileTileMax
constexpr uint32_t kPileTileMax = 1024, kPileTile = 1024;
constexpr uint32_t kPileCtrCounted = 0, kPileCtrSkipped = 1, kPileCtrBroken = 2, kPileCounters = 3;
void launch_pile_best(hipStream_t s, const DevHit* hits, uint32_t n, const uint32_t* hit_read, uint32_t n_reads, uint32_t* best);
void launch_pile_count(hipStream_t s, const DevHit* hits, uint32_t n, const uint32_t* hit_bin, const uint32_t* hit_read, uint32_t n_bins, uint32_t n_reads,
                       const uint32_t* best, uint32_t slack, uint32_t* const* bin_cnt, uint64_t* ctr);
void launch_pile(hipStream_t s, const DevHit* hits, uint32_t n, const uint32_t* hit_bin, const uint32_t* hit_read, const DevBin* bins, uint32_t n_bins,
                 uint32_t n_reads, const uint32_t* best, uint32_t slack, uint32_t* const* bin_cnt, const uint8_t* codes, const uint32_t* read_off,
                 const void* out, const uint32_t* ops, uint64_t n_ops_total, uint64_t* ctr);
void launch_pile_ref(hipStream_t s, const uint8_t* text, const uint32_t* ref_off, const uint32_t* text_start, uint32_t n_refs, uint32_t n_slots, uint8_t* ref);
uint32_t pile_tiles(uint32_t n_slots, uint32_t tile);
void launch_pile_tile_sums(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, uint32_t* tile_sum);
void launch_pile_sites_count(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, const uint32_t* tile_pre, uint32_t min_depth, uint32_t min_alt,
                             uint32_t min_alt_ppm, uint32_t* tile_cnt);
void launch_pile_sites_rows(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, const uint32_t* tile_pre, uint32_t min_depth, uint32_t min_alt,
                            uint32_t min_alt_ppm, const uint32_t* tile_off, const uint32_t* ref_off, const uint64_t* ref_key, uint32_t n_refs, const uint8_t* ref,
                            void* rows, uint64_t n_rows);
void launch_pile_dump(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, const uint32_t* tile_pre, uint32_t lo, uint32_t hi, uint32_t* dump);
// k_cons.hip: the consensus of a pileup segment, as the head of k_cons.hip defines it; cnt, tile, tile_pre, ref_off, ref_key
// and ref are k_pile.hip's.  md = max(min_depth, 1).
//   call:    cells[n_refs][kConsCell] (zeroed by the caller) += covered, n_ref, n_sub, n_del, n_low, n_ambig, ins_sites, -, and
//            sum_depth as a u64 at [8]; with call != null also call[n_slots] = the character a slot emits or 0, tile_cnt[t] = the
//            characters of tile t, ref_pre[r] = the characters of its tile in front of reference r's first slot
//   (launch_scan over tile_cnt: tile_off[0 .. tiles])
//   layout:  lay[n_refs][kConsLay] = text_off (u64), header bytes, cons_len, characters in front of the reference, emitted,
//            bytes (u64); total[0] = the text's bytes, total[1] = the emitted references.  One workgroup.
//   write:   the headers and the characters of the emitted references into text[0 .. text_bytes), which begins on a 4-byte
//            boundary; staged: tiles inside one reference put their bytes together in LDS and store whole dwords
//   add:     counts[n][8], plain, added to the n slots from `first` of a reference of `slots` slots whose counters begin at cnt;
//            first + n <= slots, and channel 0 of slot `slots - 1` is zero when it is among them
constexpr uint32_t kConsCell = 10, kConsLay = 8;
constexpr bool kConsStagedDefault = true;   // which write pass a consensus takes unless MTSV_CONS_WRITE says so: profiles/README.md
void launch_cons_call(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, const uint32_t* tile_pre, const uint32_t* ref_off, uint32_t n_refs,
                      const uint8_t* ref, uint32_t md, uint32_t min_frac_ppm, uint32_t fill, uint8_t* call, uint32_t* tile_cnt, uint32_t* ref_pre,
                      uint32_t* cells);
void launch_cons_layout(hipStream_t s, const uint32_t* cells, const uint32_t* ref_off, const uint64_t* ref_key, uint32_t n_refs, const uint32_t* ref_pre,
                        const uint32_t* tile_off, uint32_t tile, uint32_t min_breadth_ppm, uint32_t line_width, uint32_t* lay, uint64_t* total);
void launch_cons_write(hipStream_t s, const uint8_t* call, uint32_t n_slots, uint32_t tile, const uint32_t* tile_off, const uint32_t* ref_off,
                       const uint64_t* ref_key, uint32_t n_refs, const uint32_t* lay, uint32_t line_width, uint8_t* text, uint64_t text_bytes, bool staged);
void launch_cons_add(hipStream_t s, uint32_t* cnt, uint32_t slots, uint32_t first, uint64_t n, const uint32_t* counts);

}  // namespace mtsv
