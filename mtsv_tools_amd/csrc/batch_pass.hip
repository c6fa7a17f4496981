// batch_pass.hip -- the driver every read goes through: a resident range over the lanes (run_range), a slice in passes
// (run_slice), and the stages of a pass.  No kernels of its own; the counter slots and the launchers are kernels.hpp's, the
// arithmetic that cuts ranges and slices pass_plan.hpp's.  The order of launches, clears, event records, publishes and
// synchronises inside a stage is the contract ("How a pass is laid out").
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "batch.hpp"

namespace mtsv {

// A resident range of reads, split over the lanes (plan_chunks); the hits stay in the lanes, `segments` records them in
// read order.  raw != nullptr: the range is still ASCII in `raw` and each chunk normalises its bytes into
// `sb` first (h_off = host copy of the range's n + 1 offsets); raw == nullptr: `sb` already holds codes.
void Batch::run_range(const mtsv_params& p, const uint8_t* raw, uint8_t* sb, const uint32_t* so, const uint32_t* h_off, uint64_t n,
                      uint32_t range_max_len, uint64_t read_base) {
    std::vector<Batch*> ls{this};
    for (auto& l : extra) ls.push_back(l.get());
    uint64_t per_lane = 2;  // measured on config2: 1: 52.2 ms, 2: 51.9, 3: 53.0, 4: 54.7, 6: 57.0 per 10 M reads
    if (const char* e = getenv("MTSV_CHUNKS_PER_LANE")) per_lane = std::max(1, atoi(e));
    const ChunkPlan cp = plan_chunks(n, ls.size(), ws_reads, per_lane);
    const uint64_t n_chunks = cp.n_chunks(), k = cp.k;
    lanes_used = std::max<uint64_t>(lanes_used, k);
    std::vector<Segment> segs(n_chunks);
    std::atomic<uint64_t> next{0};
    auto work = [&](Batch* lane) {
        for (;;) {
            const uint64_t c = next.fetch_add(1);
            if (c >= n_chunks) return;
            const uint64_t a = cp.bound[c], b = cp.bound[c + 1];
            const uint64_t before = lane->n_hits_total, a_before = lane->n_assign_total;
            // base normalisation (binner.rs:88-100) of this chunk's bytes: raw -> codes, on the lane's stream
            if (raw) launch_normalise(lane->stream, raw, sb, h_off[a], h_off[b]);
            lane->run_slice(p, sb, so + a, h_off ? h_off + a : nullptr, b - a, range_max_len, read_base + a);
            segs[c] = Segment{lane, before, lane->n_hits_total - before, a, b - a, a_before, lane->n_assign_total - a_before};
        }
    };
    if (k == 1) {
        work(this);
    } else {
        std::vector<std::exception_ptr> errs(k);
        std::vector<std::thread> th;
        for (uint64_t i = 1; i < k; i++)
            th.emplace_back([&, i] {
                try {
                    HIP_CHECK(hipSetDevice(di->device));
                    work(ls[i]);
                } catch (...) {
                    errs[i] = std::current_exception();
                    next.store(n_chunks);  // stop the others
                }
            });
        try {
            work(this);
        } catch (...) {
            errs[0] = std::current_exception();
            next.store(n_chunks);
        }
        for (auto& t : th) t.join();
        for (auto& e : errs)
            if (e) std::rethrow_exception(e);
    }
    for (auto& sg : segs) segments.push_back(sg);
}

// One pass: reads [r0, r0 + plan.nr) of the slice, what the stages hand to each other, and the verify turn the pass holds.
struct Batch::Pass {
    const mtsv_params& p;
    const uint8_t* sb;
    const uint32_t* so;
    uint64_t read_base, r0;
    PassPlan plan;
    uint32_t nstr;           // strands: two per read
    bool tile_pass = false;  // the seed stage ran by tiles (stage_locate must follow it)
    uint64_t total_hits = 0, total_out = 0;  // seed hits (after stage_seeds), hits (after stage_gather)
    VerifyTurn::Guard turn;
};

// One slice of reads already in HBM (bases `sb`, offsets `so`, `n_slice` reads whose first read is
// number `read_base` of the caller's batch): passes over the slice, hits appended to d_hits.
// h_off: host copy of the slice's n_slice + 1 offsets (needed only when the slice holds reads beyond
// kMaxRegisterReadLen bases).
void Batch::run_slice(const mtsv_params& p, const uint8_t* sb, const uint32_t* so, const uint32_t* h_off, uint64_t n_slice,
                      uint32_t slice_max_len, uint64_t read_base) {
    if (slice_max_len > kMaxReadLen)
        throw std::runtime_error("limit: read of " + std::to_string(slice_max_len) + " bases; this build verifies reads up to " +
                                 std::to_string(kMaxReadLen));
    if (slice_max_len > kMaxRegisterReadLen && !h_off) throw std::runtime_error("internal: a slice with long reads needs its host offsets");
    uint64_t pass_reads = n_slice, r0 = 0;
    while (r0 < n_slice) {
        const PassPlan pl = plan_pass(h_off, r0, pass_reads, n_slice, slice_max_len, p.seed_size, p.seed_interval, verify_mode, sw_pairs, hit_cap);
        Pass ps{p, sb, so, read_base, r0, pl, pl.nr * 2};
        room_seed_slots(pl);
        room_planes(pl);
        const Seeded seeded = stage_seeds(ps);
        if (seeded == Seeded::kHalfReads) pass_reads = std::max<uint64_t>(1, pl.nr / 2);
        if (seeded != Seeded::kGoOn) continue;  // the pass again: nothing of it has been counted
        stats.n_passes++;
        stats.n_seed_tile_passes += ps.tile_pass;
        if (getenv("MTSV_TRACE")) fprintf(stderr, "[lane] pass of %u reads, max_ns %u, longest read %u: seed stage %s\n", pl.nr, pl.max_ns, pl.pass_max_len, ps.tile_pass ? "by tiles" : "legacy");
        stats.n_seed_slots += pl.slots;
        stats.n_seed_hits += ps.total_hits;
        stage_locate(ps);
        stage_candidates(ps);
        stage_verify(ps);
        stage_gather(ps);
        stage_commit(ps);
        n_hits_total += ps.total_out;
        for (int s = 0; s < 7; s++) {
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, ev[s], ev[s + 1]));
            stage_acc[s] += ms;
        }
        r0 += pl.nr;
    }
}

void Batch::room_seed_slots(const PassPlan& pl) {
    if (pl.slots <= seed_cap) return;
    const uint64_t had = seed_cap;
    seed_cap = 0;
    release_all(d_seed_lo, d_seed_cnt, d_seed_pre);
    // room for a full workspace of reads like these, not just this pass: slices of a host batch grow
    // towards the workspace size, and every hipFree / hipMalloc stalls the whole device
    const uint64_t want = pl.tiled() ? pl.slots : std::max<uint64_t>(pl.slots, 2 * ws_reads * (uint64_t)pl.max_ns);
    if (getenv("MTSV_TRACE")) fprintf(stderr, "[workspace] seed slot arrays grow %llu -> %llu entries\n", (unsigned long long)had, (unsigned long long)want);
    d_seed_lo.alloc(want, "seed slots: ranges");
    d_seed_cnt.alloc(want, "seed slots: counts");
    d_seed_pre.alloc(want, "seed slots: prefix sums");
    seed_cap = want;
}

// the reads' bit planes (EvalArgs::planes) for the passes k_edit_myers verifies: k_thin writes them, sized like
// the seed slot arrays for a full workspace of reads like these
void Batch::room_planes(const PassPlan& pl) {
    if ((uint64_t)pl.nr * 3 * pl.plane_words <= d_planes.cap) return;
    d_planes.renew(std::max<uint64_t>(pl.nr, ws_reads) * 3 * pl.plane_words, "the reads' bit planes");
}

void Batch::room_strip(uint64_t need) {
    if (need <= d_strip.cap) return;
    d_strip.renew(need, "the band strips");
}

// the result array grows, keeping what earlier passes produced
void Batch::room_hits(uint64_t total_out) {
    if (n_hits_total + total_out <= d_hits.cap) return;
    DevBuf<DevHit> grown;  // (a failure leaves the lane as it was; the old array leaves with this one)
    grown.alloc(std::max(d_hits.cap * 2, n_hits_total + total_out), "the result array");
    if (n_hits_total) HIP_CHECK(hipMemcpyAsync(grown.p, d_hits.p, n_hits_total * sizeof(DevHit), hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    // run_host may be copying an earlier slice's hits out of the old array on the owner's copy stream (and
    // another lane's thread may be issuing such a copy right now: the commit mutex covers the pointer swap)
    std::unique_lock<std::mutex> commit_lk;
    if (root()->commit_mu) commit_lk = std::unique_lock<std::mutex>(*root()->commit_mu);
    if (root()->copy_stream2) HIP_CHECK(hipStreamSynchronize(root()->copy_stream2));
    d_hits.swap(grown);
}

// ---- seeds: search, thin, scan; the pass's first round trip.  Nothing here touches the statistics.
Batch::Seeded Batch::stage_seeds(Pass& ps) {
    const PassPlan& pl = ps.plan;
    const mtsv_params& p = ps.p;
    const uint32_t K = p.seed_size, G = p.seed_interval, r0 = (uint32_t)ps.r0;
    uint32_t* planes = pl.myers() ? d_planes.p : nullptr;
    HIP_CHECK(hipEventRecord(ev[kEvPassBegin], stream));
    // (d_seed_pre is k_thin's output: until then it holds the list of the slots that take the general code -- an N in
    //  the seed's table part; counter kCtrListedSlots.  The second kernel's grid covers the share of such slots the passes
    //  before had, half as much again: the count is checked at the round trip below.)
    const uint32_t listed_cap = (uint32_t)std::min<uint64_t>(pl.slots, std::max<uint64_t>(4096, (uint64_t)((double)pl.slots * listed_share)));
    launch_search(stream, di->view, ps.sb, ps.so, r0, pl.nr, pl.max_ns, K, G, d_seed_lo.p, d_seed_cnt.p, d_seed_pre.p, (uint32_t*)(d_counters.p + kCtrListedSlots),
                  listed_cap, di->d_kmer_levels, fused_clear && listed_zero);
    listed_zero = false;
    HIP_CHECK(hipEventRecord(ev[kEvSearched], stream));
    // the seed stage by tiles when the pass fits them (kernels.hpp); k_thin and k_expand with seed_pre between them otherwise
    ps.tile_pass = seed_tiles && pl.max_ns && seed_tile_fits(pl.max_ns, pl.pass_max_len, pl.slots);
    if (ps.tile_pass)
        launch_thin_tiled(stream, ps.sb, ps.so, r0, pl.nr, p.edit_rate, p.min_seed, pl.max_ns, K, G, p.max_hits, p.tune_max_hits, d_seed_cnt.p,
                          d_strand_hits.p, d_strand_nseeds.p, planes, pl.plane_words);
    else if (pl.max_ns)
        launch_thin(stream, ps.sb, ps.so, r0, pl.nr, p.edit_rate, p.min_seed, pl.max_ns, K, G, p.max_hits, p.tune_max_hits, d_seed_cnt.p,
                    d_seed_pre.p, d_strand_hits.p, d_strand_nseeds.p, planes, pl.plane_words);
    else {
        HIP_CHECK(hipMemsetAsync(d_strand_hits.p, 0, (uint64_t)ps.nstr * 4, stream));
        HIP_CHECK(hipMemsetAsync(d_strand_nseeds.p, 0, (uint64_t)ps.nstr * 4, stream));
    }
    launch_scan(stream, d_strand_hits.p, ps.nstr, d_tile_sums.p, d_counters.p + kCtrSeedHits, d_strand_off.p);
    launch_publish(stream, d_counters.p + kCtrSeedHits, h_counters.p + kCtrSeedHits, 1);
    launch_publish(stream, d_counters.p + kCtrListedSlots, h_counters.p + kCtrListedSlots, 1);
    HIP_CHECK(hipEventRecord(ev[kEvSeeded], stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const uint64_t n_listed = h_counters.p[kCtrListedSlots] & 0xffffffffull;
    const double share = pl.slots ? (double)n_listed / (double)pl.slots : 0.0;
    if (n_listed > listed_cap) {  // more slots on the list than the grid covered: the pass again, with a grid for them
        listed_share = std::min(1.0, share * 1.25 + 0.01);
        if (getenv("MTSV_TRACE")) fprintf(stderr, "[lane] %llu listed seed slots, grid for %u: pass again\n", (unsigned long long)n_listed, listed_cap);
        return Seeded::kSameReads;
    }
    listed_share = std::min(1.0, std::max(0.02, share * 1.5 + 0.005));
    ps.total_hits = h_counters.p[kCtrSeedHits];
    if (ps.total_hits > hit_cap) {
        if (pl.nr > 1) return Seeded::kHalfReads;  // redo this pass with fewer reads
        // one read with more seed hits than the workspace (a long read in a repeat): grow the workspace
        if (ps.total_hits > 0xfffffff0ull)
            throw std::runtime_error("device: one read has " + std::to_string(ps.total_hits) + " seed hits, more than 2^32");
        grow_hit_workspace(ps.total_hits);
    }
    return Seeded::kGoOn;
}

// ---- locate: the kept seeds' SA rows, then their text positions
void Batch::stage_locate(Pass& ps) {
    const DevIndexView& v = di->view;
    if (ps.tile_pass)
        launch_expand_tiled(stream, v, ps.nstr, ps.plan.max_ns, ps.p.seed_interval, d_seed_lo.p, d_seed_cnt.p, d_strand_off.p, d_hit_row.p, d_hit_ref.p, d_hit_q.p);
    else
        launch_expand(stream, v, ps.nstr, ps.plan.max_ns, ps.p.seed_interval, d_seed_lo.p, d_seed_cnt.p, d_seed_pre.p, d_strand_off.p, d_hit_row.p, d_hit_ref.p,
                      d_hit_q.p);
    HIP_CHECK(hipEventRecord(ev[kEvExpanded], stream));
    if (!v.sa_full)
        launch_locate(stream, v, (uint32_t)ps.total_hits, d_strand_off.p + ps.nstr, d_hit_row.p, d_hit_ref.p,
                      (unsigned long long*)(d_counters.p + kCtrLfSteps));
    HIP_CHECK(hipEventRecord(ev[kEvLocated], stream));
}

// ---- candidates: the coalescing kernels
void Batch::stage_candidates(Pass& ps) {
    // One launch zeroes the counters these kernels start from, k_coalesce_heavy's ticket, the counters round 0 of the verify
    // rounds starts from (no coalescing kernel touches them) and k_search's list count of the next pass (the host has read it).
    if (fused_clear) {
        launch_clear_counters(stream, d_counters.p, kCtrClearPass | (ps.plan.path == VerifyPath::kRounds ? kCtrClearRound0 : 0));
        listed_zero = true;
    } else {
        HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrWorklist, 0, 8, stream));
        HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrWlCursor, 0, 8, stream));
        HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrMidStrands, 0, 8, stream));
    }
    launch_coalesce(stream, di->view, ps.so, (uint32_t)ps.r0, ps.nstr, ps.p.max_candidates, d_strand_off.p,
                    d_strand_nseeds.p, d_hit_ref.p, d_hit_q.p, d_hit_key.p, d_cand_tmp.p, d_cand.p, d_cand_next.p,
                    d_cand_status.p, d_strand_ncand.p, d_worklist.p, d_heavy_list.p, d_counters.p, fused_clear);
    HIP_CHECK(hipEventRecord(ev[kEvCoalesced], stream));
}

// ---- verify: one of the four paths, then the selection
// One lane of the workspace at a time (the turn): this lane's coalescing kernels are enqueued and run while it waits,
// beside the verify kernels of the lane that has it.  It goes back after the pass's last verify round trip, or with
// whatever leaves this pass early.  (A pass without seed hits does not take it; its kernels are still launched, at
// their smallest grids, and find nothing.)
void Batch::stage_verify(Pass& ps) {
    const DevIndexView& v = di->view;
    const PassPlan& pl = ps.plan;
    if (ps.total_hits) ps.turn.take(root()->verify_turn, ps.read_base + ps.r0, this);
    EvalArgs a;
    a.bases = ps.sb;
    a.read_off = ps.so;
    a.r0 = (uint32_t)ps.r0;
    a.edit_rate = ps.p.edit_rate;
    a.max_candidates = ps.p.max_candidates;
    a.strand_off = d_strand_off.p;
    a.cand = d_cand.p;
    a.cand_next = d_cand_next.p;
    a.cand_status = d_cand_status.p;
    a.planes = pl.myers() ? d_planes.p : nullptr;
    a.plane_words = pl.plane_words;
    a.out = d_out.p;
    a.n_verified = (unsigned long long*)(d_counters.p + kCtrVerified);
    a.window_bytes = (unsigned long long*)(d_counters.p + kCtrWindowBytes);
    a.sw_columns = (unsigned long long*)(d_counters.p + kCtrSwCellPairs);
    // one launch: a group whose candidate fails walks on to the next candidate of the same TaxId
    a.worklist = d_worklist.p;
    a.wl_count = (const uint32_t*)(d_counters.p + kCtrWorklist);
    a.wl_cursor = (uint32_t*)(d_counters.p + kCtrWlCursor);
    stats.n_rounds = 1;
    switch (pl.path) {
        case VerifyPath::kTiled: verify_tiled(ps, a); break;
        case VerifyPath::kEditFirst: root()->verify_turn.note_grid(launch_edit_myers(stream, v, a, ps.total_hits, pl.pass_max_len, 0, root()->myers_wgs_per_cu, false, root()->myers_fetch_legacy)); break;
        case VerifyPath::kRounds: verify_rounds(ps, a); break;
        case VerifyPath::kPacked: launch_evaluate(stream, v, a, ps.total_hits, pl.pass_max_len); break;
    }
    // (flags only: whether a strand has a hit does not depend on max_assignments -- the loop of index.rs:384-428
    //  pushes its first accepted candidate before it looks at the limit -- so the selection stops at the first)
    launch_resolve(stream, ps.nstr, ps.p.max_candidates, flags_only() ? 1 : ps.p.max_assignments, d_strand_off.p, d_strand_ncand.p, d_cand_status.p,
                   d_out.p, d_strand_nout.p);
    HIP_CHECK(hipEventRecord(ev[kEvVerified], stream));
}

// strips sized from the longest window of the pass (one small round trip; long reads are rare)
void Batch::verify_tiled(Pass& ps, EvalArgs& a) {
    HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrMaxWindow, 0, sizeof(uint64_t), stream));
    launch_max_window(stream, ps.nstr, d_strand_off.p, d_strand_ncand.p, d_cand.p, (unsigned long long*)(d_counters.p + kCtrMaxWindow));
    launch_publish(stream, d_counters.p + kCtrMaxWindow, h_counters.p + kCtrMaxWindow, 1);
    HIP_CHECK(hipStreamSynchronize(stream));
    const uint32_t strip_len = (uint32_t)std::max<uint64_t>(h_counters.p[kCtrMaxWindow], 1);
    room_strip((uint64_t)tiled_groups(ps.total_hits, strip_len) * strip_len);
    a.strip = d_strip.p;
    a.strip_len = strip_len;
    launch_evaluate_tiled(stream, di->view, a, ps.total_hits);
}

// One verify round: what its front-ends hand to the common tail.
struct Batch::Round {
    uint32_t round = 0;
    uint64_t items = 0;        // entries of the round's work list, at most
    uint64_t tail_items = 0;   // ... of the list the tail works on, at most (tail_listed: exactly, known on the host)
    bool tail_listed = false;
    bool fused = false;        // round 0 is k_edit_myers in fused mode
    EvalArgs sw;               // k_sw_pairs' arguments: the front-ends of round 0 move its work list on
    uint32_t *pass_list = nullptr, *sweep_list = nullptr, *next_list = nullptr;
    uint64_t* next_slot = nullptr;  // kCtrNext0 or kCtrNext1: the count of next_list
};

// Reference order, split by predicate: k_sw_pairs runs the prefilter of index.rs:406 two candidates per group, k_edit_myers
// the edit distance of :407-410 on those that passed.  A candidate that passes the first and fails the second sends its
// TaxId's next candidate to another round (rare); rounds end when nothing is left.
// Round 0 is one pass of k_edit_myers in fused mode over the whole worklist: the unit-cost distance under the SW matrix's
// matches decides the prefilter from both sides and, wherever read or window holds no N, is the edit distance itself.
// k_sw_pairs sweeps what lies between its thresholds, list mode finishes what the sweep passed.  MTSV_SW_FUSED=0 (and
// MTSV_SW_BOUND=0) start with k_sw_diag instead: the lower bounds on the seed diagonal, a lane per work item; what they decide
// goes straight to pass_list, the rest to sweep_list for k_sw_pairs.
void Batch::verify_rounds(Pass& ps, const EvalArgs& a) {
    Round r;
    r.fused = sw_bound && sw_fused;
    r.pass_list = (uint32_t*)d_hit_key.p;              // coalesce scratch is free now
    r.sweep_list = (uint32_t*)d_hit_key.p + hit_cap;   // (8 bytes per seed hit)
    uint32_t* next_lists[2] = {(uint32_t*)d_cand_tmp.p, (uint32_t*)d_cand_tmp.p + hit_cap};
    const uint32_t* wl = d_worklist.p;
    uint32_t wl_slot = kCtrWorklist;  // the slot whose low word is wl's length
    r.items = ps.total_hits;
    for (;; r.round++) {
        r.next_slot = d_counters.p + kCtrNext0 + (r.round & 1);
        r.next_list = next_lists[r.round & 1];
        if (!fused_clear) {
            HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrSwCursor, 0, 3 * sizeof(uint64_t), stream));
            HIP_CHECK(hipMemsetAsync(r.next_slot, 0, sizeof(uint64_t), stream));
        } else if (r.round) {  // (round 0: zeroed with the coalescing kernels' counters)
            launch_clear_counters(stream, d_counters.p, ctr_clear_round(r.round));
        }
        // The tail of a round -- k_sw_pairs and list-mode k_edit_myers -- is sized from its own list: later rounds
        // have its length on the host (n_next); round 0 asks for what the fused pass left undecided, one more round
        // trip in place of two persistent grids sized from the pass's seed hits.  An empty list launches nothing.
        r.tail_items = r.items;
        r.tail_listed = tail_from_list && r.round > 0;
        r.sw = a;
        r.sw.worklist = wl;
        r.sw.wl_count = (const uint32_t*)(d_counters.p + wl_slot);
        r.sw.wl_cursor = (uint32_t*)(d_counters.p + kCtrSwCursor);
        r.sw.wl_reverse = r.round == 0;
        r.sw.counters = d_counters.p;
        r.sw.wl_count_slot = wl_slot;
        r.sw.pass_list = r.pass_list;
        r.sw.pass_count = (uint32_t*)(d_counters.p + kCtrPassCount);
#ifdef MTSV_SW_HIST
        if (!d_strip.p) room_strip(4096);
        HIP_CHECK(hipMemsetAsync(d_strip.p, 0, 768 * 4, stream));
        r.sw.strip = d_strip.p;
#endif
        if (r.round == 0) {
            HIP_CHECK(hipEventRecord(ev[kEvSwBegin], stream));
            if (sw_diag && sw_prepass && !r.fused) round0_diag(ps, r);
            if (sw_bound) round0_bound(ps, r);
            else if (sw_diag && sw_prepass && sw_top) round0_top(ps, r);
        }
        round_tail(ps, r, a);
        if (r.round == 0) round0_times();
        const uint64_t n_next = h_counters.p[kCtrNext0] & 0xffffffffull;  // (either slot is published there)
        if (n_next == 0) break;
        stats.n_rounds++;
        wl = r.next_list;
        wl_slot = kCtrNext0 + (r.round & 1);
        r.items = n_next;
    }
    ps.turn.release();
}

// round 0 without the fused pass: the lower bounds on the seed diagonal first
void Batch::round0_diag(Pass& ps, Round& r) {
    HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrSweepCount, 0, sizeof(uint64_t), stream));
    launch_sw_diag(stream, di->view, r.sw, r.items, ps.plan.pass_max_len, r.sweep_list, kCtrSweepCount);
    HIP_CHECK(hipEventRecord(ev[kEvDiagEnd], stream));
    r.sw.worklist = r.sweep_list;
    r.sw.wl_count_slot = kCtrSweepCount;
    r.sw.wl_reverse = 0;  // k_sw_diag read the worklist from its end
}

// What the lower bounds leave are mostly chance seed hits.  The unit-cost edit distance under the SW matrix's matches bounds
// the score from both sides (k_edit_myers in bound mode) at a third of a sweep's instructions: it refutes those, passes most
// of the rest, and only what lies between its two thresholds (kCtrUndecided counts it; the seed-hit rows of k_expand are free
// by now) is swept by the tail.
void Batch::round0_bound(Pass& ps, Round& r) {
    if (!fused_clear) HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrUndecided, 0, 2 * sizeof(uint64_t), stream));  // and kCtrBoundCursor
    EvalArgs bd = r.sw;
    bd.wl_count = (const uint32_t*)(d_counters.p + r.sw.wl_count_slot);
    bd.wl_cursor = (uint32_t*)(d_counters.p + kCtrBoundCursor);
    bd.und_list = (uint32_t*)d_hit_row.p;
    bd.und_slot = kCtrUndecided;
    bd.myers_ctr = (unsigned long long*)(d_counters.p + kCtrMyersColumns);
    // (fused: from the worklist's end, and accepted candidates go straight to `out`)
    root()->verify_turn.note_grid(launch_edit_myers(stream, di->view, bd, r.items, ps.plan.pass_max_len, r.fused ? 3 : 2, root()->myers_wgs_per_cu, false, root()->myers_fetch_legacy));
    HIP_CHECK(hipEventRecord(ev[kEvBoundEnd], stream));
    r.sw.worklist = bd.und_list;
    r.sw.wl_count_slot = kCtrUndecided;
    r.sw.wl_reverse = 0;
    if (r.fused && tail_from_list) {  // (fused: the pass list holds only what k_sw_pairs passes of these)
        launch_publish(stream, d_counters.p + kCtrUndecided, h_counters.p + kCtrUndecided, 1);
        HIP_CHECK(hipStreamSynchronize(stream));
        r.tail_items = h_counters.p[kCtrUndecided] & 0xffffffffull;
        r.tail_listed = true;
    }
}

// (MTSV_SW_BOUND=0) most of these are refuted on the top half of the read rows; the full-height launch of the tail takes
// what is left (kCtrUndecided counts it)
void Batch::round0_top(Pass& ps, Round& r) {
    HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrUndecided, 0, sizeof(uint64_t), stream));
    r.sw.und_list = (uint32_t*)d_hit_row.p;
    r.sw.und_slot = kCtrUndecided;
    launch_sw_pairs(stream, di->view, r.sw, r.items, ps.plan.pass_max_len, false, true);
    HIP_CHECK(hipMemsetAsync(d_counters.p + kCtrSwCursor, 0, sizeof(uint64_t), stream));  // the claim cursor
    r.sw.worklist = r.sw.und_list;
    r.sw.wl_count_slot = kCtrUndecided;
}

// the common tail of a round: k_sw_pairs, list-mode k_edit_myers, and the round trip that tells what passed and what is next
void Batch::round_tail(Pass& ps, Round& r, const EvalArgs& a) {
    const DevIndexView& v = di->view;
    const uint32_t max_len = ps.plan.pass_max_len;
    const bool first = r.round == 0, tail_empty = r.tail_listed && r.tail_items == 0;
    if (!tail_empty) launch_sw_pairs(stream, v, r.sw, r.tail_items, max_len, sw_diag, false, first && sw_bound && !r.tail_listed);
#ifdef MTSV_SW_HIST
    {
        static uint32_t hh[768];
        HIP_CHECK(hipMemcpyAsync(hh, d_strip.p, sizeof hh, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        fprintf(stderr, "SWHIST round %u steps/4:", r.round);
        for (int i = 0; i < 128; i++) if (hh[i]) fprintf(stderr, " %d:%u", i * 4, hh[i]);
        fprintf(stderr, "\nSWHIST halves sweeping 0/1/2: %u %u %u\nSWHIST fail best:", hh[128], hh[129], hh[130]);
        for (int i = 0; i < 256; i++) if (hh[256 + i]) fprintf(stderr, " %d:%u", i, hh[256 + i]);
        fprintf(stderr, "\nSWHIST pass best:");
        for (int i = 0; i < 256; i++) if (hh[512 + i]) fprintf(stderr, " %d:%u", i, hh[512 + i]);
        fprintf(stderr, "\n");
    }
#endif
    if (first) HIP_CHECK(hipEventRecord(ev[kEvSwEnd], stream));
    EvalArgs my = a;
    my.worklist = r.pass_list;
    my.wl_count = (const uint32_t*)(d_counters.p + kCtrPassCount);
    my.wl_cursor = (uint32_t*)(d_counters.p + kCtrMyersCursor);
    my.next_list = r.next_list;
    my.next_count = (uint32_t*)r.next_slot;
    my.myers_ctr = (unsigned long long*)(d_counters.p + kCtrMyersColumns);
    if (!tail_empty) root()->verify_turn.note_grid(launch_edit_myers(stream, v, my, r.tail_items, max_len, 1, root()->myers_wgs_per_cu, r.tail_listed, root()->myers_fetch_legacy));
    if (first) HIP_CHECK(hipEventRecord(ev[kEvEditEnd], stream));
    if (tail_empty) {
        h_counters.p[kCtrPassCount] = h_counters.p[kCtrNext0] = 0;  // nothing passed, nothing for another round
        if (first) HIP_CHECK(hipEventSynchronize(ev[kEvEditEnd]));
    } else {
        launch_publish(stream, r.next_slot, h_counters.p + kCtrNext0, 1);
        launch_publish(stream, d_counters.p + kCtrPassCount, h_counters.p + kCtrPassCount, 1);
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    sw_passed_acc += h_counters.p[kCtrPassCount] & 0xffffffffull;
}

// round 0's device times by kernel family, from the events its kernels were bracketed with
void Batch::round0_times() {
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[kEvSwBegin], ev[kEvSwEnd]));
    sw_ms_acc += ms;
    int from = kEvSwBegin;  // the sweeps start after whichever bound kernels ran
    if (sw_diag && sw_prepass && !(sw_bound && sw_fused)) {
        HIP_CHECK(hipEventElapsedTime(&ms, ev[kEvSwBegin], ev[kEvDiagEnd]));
        diag_ms_acc += ms;
        from = kEvDiagEnd;
    }
    if (sw_bound) {
        HIP_CHECK(hipEventElapsedTime(&ms, ev[from], ev[kEvBoundEnd]));
        bound_ms_acc += ms;
        from = kEvBoundEnd;
    }
    HIP_CHECK(hipEventElapsedTime(&ms, ev[from], ev[kEvSwEnd]));
    sweep_ms_acc += ms;
    HIP_CHECK(hipEventElapsedTime(&ms, ev[kEvSwEnd], ev[kEvEditEnd]));
    edit_ms_acc += ms;
}

// ---- gather: the pass's hits behind those of the passes before, in (read, strand, rank) order
// (flags only: no scan of the hit counts, no result array, no gather -- the pass ends with k_match)
void Batch::stage_gather(Pass& ps) {
    const bool only_flags = flags_only();
    if (!only_flags) {
        launch_scan(stream, d_strand_nout.p, ps.nstr, d_tile_sums.p, d_counters.p + kCtrOutTotal, d_out_off.p);
        launch_publish(stream, d_counters.p, h_counters.p, kCtrWlCursor + 1);
        HIP_CHECK(hipStreamSynchronize(stream));
        ps.total_out = h_counters.p[kCtrOutTotal];
        ps.turn.release();  // (the paths without rounds: their verify kernels are through)
    }
    room_hits(ps.total_out);
    if (!only_flags) launch_gather(stream, ps.nstr, ps.read_base + ps.r0, d_strand_off.p, d_strand_nout.p, d_out_off.p, d_out.p, d_hits.p, n_hits_total);
    // (a compacted batch: the hits carry the caller's read numbers; the report and the flags are per resident read)
    if (!only_flags && root()->mapped) launch_remap_reads(stream, d_hits.p + n_hits_total, ps.total_out, root()->d_read_map.p);
    HIP_CHECK(hipEventRecord(ev[kEvGathered], stream));
}

// ---- commit: the pass is committed from here on (a pass that is run again has not come this far): its reads join the taxa
// report, get their match flags, and their hits are reduced to assignments; the pass's last synchronise
void Batch::stage_commit(Pass& ps) {
    const uint32_t nr = ps.plan.nr;
    TaxaReport& rep = root()->report;
    if (rep.on) {
        if (!report_ev.created()) report_ev.create();
        HIP_CHECK(hipEventRecord(report_ev[0], stream));
        launch_report(stream, nr, d_strand_nout.p, d_out_off.p, d_hits.p + n_hits_total, rep.d_taxa.p, rep.n_taxa, rep.dense, rep.hash_slots, rep.d_counts.p,
                      rep.d_counts.p + 4ull * rep.n_taxa, rep.trace ? rep.d_counts.p + 4ull * rep.n_taxa + 1 : nullptr);
        HIP_CHECK(hipEventRecord(report_ev[1], stream));
    }
    MatchFlags& mf = root()->match;
    if (mf.mode != MTSV_MATCH_OFF) {
        const uint64_t first_bit = ps.read_base + ps.r0 - mf.call_base;
        if (first_bit + nr > mf.n_reads) throw std::runtime_error("internal: match flags of a pass beyond the run's reads");
        if (!match_ev.created()) match_ev.create();
        HIP_CHECK(hipEventRecord(match_ev[0], stream));
        launch_match(stream, nr, d_strand_nout.p, first_bit, mf.d_words.p, mf.d_words.p + mf.cap_words());
        HIP_CHECK(hipEventRecord(match_ev[1], stream));
    }
    const bool collapse_on = !flags_only() && root()->assign.mode != MTSV_ASSIGN_OFF;
    if (collapse_on) collapse_enqueue(nr, d_strand_nout.p, d_out_off.p, d_hits.p + n_hits_total, ps.total_out);
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    ps.turn.release();
    if (collapse_on) collapse_commit();
    if (mf.mode != MTSV_MATCH_OFF) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, match_ev[0], match_ev[1]));
        std::lock_guard<std::mutex> lk(mf.mu);
        mf.ms += ms;
        mf.launches++;
    }
    if (rep.on) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, report_ev[0], report_ev[1]));
        std::lock_guard<std::mutex> lk(rep.mu);
        rep.ms += ms;
        rep.launches++;
    }
}

}  // namespace mtsv
