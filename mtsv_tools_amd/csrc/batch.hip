// batch.hip -- device workspace for one batch of reads; batch_pass.hip is the stage-by-stage driver of the hot
// path, batch_host.hip the run of a batch that lies in host memory.  Replaces the producer -> workers -> joiner
// queue of vendor/cue/src/lib.rs:45-105 with large HBM-resident batches: reads stay on the device between stages,
// every stage is one launch over the whole batch, and the only host round-trips are two 8-byte totals per pass.
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "batch.hpp"

namespace mtsv {

// true when [p, p + bytes) is page-locked host memory the runtime knows (hipHostMalloc / hipHostRegister)
bool host_pinned(const void* p, uint64_t bytes) {
    if (!p || !bytes) return false;
    for (const uint8_t* q : {(const uint8_t*)p, (const uint8_t*)p + bytes - 1}) {
        hipPointerAttribute_t at;
        memset(&at, 0, sizeof at);
        if (hipPointerGetAttributes(&at, q) != hipSuccess) {
            (void)hipGetLastError();  // ordinary memory: not an error of ours
            return false;
        }
        if (at.type != hipMemoryTypeHost) return false;
    }
    return true;
}

void* host_pinned_alloc(uint64_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void host_pinned_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}
bool host_pinned_register(void* p, uint64_t bytes) {
    if (hipHostRegister(p, bytes, hipHostRegisterPortable) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}
bool host_pinned_unregister(void* p) {
    if (hipHostUnregister(p) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

int g_default_verify_mode = MTSV_VERIFY_REFERENCE;

constexpr uint32_t kMyersWgsPerCuLanes = 3;  // k_edit_myers workgroups per CU on a workspace of several lanes (4: 0.44 ms per step slower, profiles/README.md r10)
constexpr uint64_t kChunkMaxReads = 4ull << 20;  // lanes take a range in chunks of at most this many reads (smaller chunks measured slower: per-pass launches and host round trips)

Batch::Batch(mtsv_index* ix_, DeviceIndex* di_, uint64_t max_reads_, uint64_t max_bases_, uint64_t hit_cap_, Batch* parent_, int lanes_)
    : ix(ix_), di(di_), max_reads(max_reads_), max_bases(max_bases_), hit_cap(hit_cap_), parent(parent_) {
    if (max_reads == 0) max_reads = 1;
    if (max_reads > 0x7fffffffull) throw std::runtime_error("limit: more than 2^31 reads in one batch");
    if (max_bases >= 0xffffffffull) throw std::runtime_error("limit: 4 GiB of bases or more in one batch");
    const uint64_t hit_cap_user = hit_cap;
    if (!parent) {
        n_lanes = 3;
        if (lanes_ > 0) n_lanes = std::min(8, lanes_);
        else if (const char* e = getenv("MTSV_LANES")) n_lanes = std::max(1, std::min(8, atoi(e)));
        if (max_reads < (uint64_t)n_lanes * kLaneMinReads) n_lanes = 1;
    }
    ws_reads = (max_reads + n_lanes - 1) / n_lanes;
    if (!parent && n_lanes > 1) {
        uint64_t cmax = kChunkMaxReads;
        if (const char* e = getenv("MTSV_CHUNK")) cmax = std::max<uint64_t>(kLaneMinReads, strtoull(e, nullptr, 10));
        ws_reads = std::min(ws_reads, cmax);
    }
    if (hit_cap == 0) hit_cap = std::max<uint64_t>(1ull << 20, 32 * ws_reads);
    if (hit_cap > 0xfffffff0ull) hit_cap = 0xfffffff0ull;
    uint64_t hits_cap = std::max<uint64_t>(1ull << 20, 16 * ws_reads);
    if (const char* e = getenv("MTSV_HITS_CAP")) hits_cap = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));  // (tests: initial size)
    // the device before the first member allocates: whatever throws from here on frees what exists, on that device
    HIP_CHECK(hipSetDevice(di->device));
    stream.create(hipStreamNonBlocking);
    const uint64_t ns = 2 * ws_reads;
    if (!parent) {
        d_bases.alloc(max_bases + 64, "the resident bases");  // k_search reads up to 36 bytes past a seed start with dword loads
        d_read_off.alloc(max_reads + 1, "the resident read offsets");
        d_codes.alloc(max_bases + 64, "the resident codes");  // normalised copy of d_bases, rewritten by every run()
    }
    d_strand_hits.alloc(ns + 1, "strands: seed hits");
    d_strand_nseeds.alloc(ns, "strands: seeds kept");
    d_strand_off.alloc(ns + 1, "strands: seed-hit offsets");
    d_strand_ncand.alloc(ns, "strands: candidates");
    d_strand_nout.alloc(ns + 1, "strands: hits");
    d_heavy_list.alloc(2 * ns, "strands: lists");  // [0, ns): the two strand lists of the coalescing kernels (front / back), [ns, 2 ns): the 13..16-hit strands
    d_out_off.alloc(ns + 1, "strands: hit offsets");
    d_tile_sums.alloc((uint64_t)scan_tiles((uint32_t)ns) + 1, "the scans' tile sums");
    d_counters.alloc(kCounters, "the pass counters");
    hit_cap_first = hit_cap;
    size_hit_workspace(hit_cap_first);
    d_hits.alloc(hits_cap, "the result array");
    // page-locked and mapped: kernels store the counters the host waits for straight into it (launch_publish) -- a
    // hipMemcpyAsync of 8 bytes can queue on a copy engine behind tens of milliseconds of the reads' own transfer
    h_counters.renew(kCounters, hipHostMallocMapped);
    if (const char* e = getenv("MTSV_SW")) sw_pairs = strcmp(e, "packed") != 0;
    if (const char* e = getenv("MTSV_SW_DIAG")) sw_diag = atoi(e) != 0;
    if (const char* e = getenv("MTSV_SW_PREPASS")) sw_prepass = atoi(e) != 0;
    if (const char* e = getenv("MTSV_SW_TOP")) sw_top = atoi(e) != 0;
    if (const char* e = getenv("MTSV_SW_BOUND")) sw_bound = atoi(e) != 0;
    if (const char* e = getenv("MTSV_SW_FUSED")) sw_fused = atoi(e) != 0;
    verify_mode = g_default_verify_mode;
    if (const char* e = getenv("MTSV_VERIFY")) verify_mode = !strcmp(e, "edit_first") ? 1 : 0;
    if (!parent) {
        // (measured on config2, profiles/README.md r10)
        myers_wgs_per_cu = n_lanes > 1 ? kMyersWgsPerCuLanes : kMyersWgsPerCuMax;
        if (const char* e = getenv("MTSV_MYERS_WGS_PER_CU")) myers_wgs_per_cu = (uint32_t)std::max(1, std::min((int)kMyersWgsPerCuMax, atoi(e)));
        verify_turn.on = n_lanes > 1;
        if (const char* e = getenv("MTSV_VERIFY_TURN")) verify_turn.on = verify_turn.on && atoi(e) != 0;
        if (const char* e = getenv("MTSV_TAIL_FROM_LIST")) tail_from_list = atoi(e) != 0;
        if (const char* e = getenv("MTSV_FUSED_CLEAR")) fused_clear = atoi(e) != 0;
        if (const char* e = getenv("MTSV_SEED_STAGE")) seed_tiles = strcmp(e, "legacy") != 0;
        if (const char* e = getenv("MTSV_MYERS_FETCH")) myers_fetch_legacy = strcmp(e, "legacy") == 0;
    } else {
        myers_wgs_per_cu = parent->myers_wgs_per_cu;
        tail_from_list = parent->tail_from_list;
        fused_clear = parent->fused_clear;
        seed_tiles = parent->seed_tiles;
        myers_fetch_legacy = parent->myers_fetch_legacy;
    }
    ev.create();
    for (int k = 1; k < n_lanes; k++) extra.emplace_back(new Batch(ix, di, ws_reads, 0, hit_cap_user, this));
}

// The lanes first: they borrow the owner's inputs.  The members free themselves after this body, on the device it sets; the
// two pinned stages return their arrays to the pool then, after the streams that filled them have been waited for here.
Batch::~Batch() {
    extra.clear();
    (void)hipSetDevice(di->device);
    for (hipStream_t s : {stream.s, copy_stream.s, copy_stream2.s})
        if (s) (void)hipStreamSynchronize(s);
}

// the arrays indexed by seed hit / candidate; nothing of a pass lives in them before its locate stage
void Batch::size_hit_workspace(uint64_t cap) {
    hit_cap = 0;
    release_all(d_hit_row, d_hit_ref, d_hit_q, d_hit_key, d_cand_tmp, d_cand, d_out, d_cand_next, d_cand_status, d_worklist);
    d_hit_row.alloc(cap, "hit workspace: rows");
    d_hit_ref.alloc(cap, "hit workspace: references");
    d_hit_q.alloc(cap, "hit workspace: read positions");
    d_hit_key.alloc(cap, "hit workspace: keys");
    d_cand_tmp.alloc(2 * cap, "hit workspace: candidate scratch");
    d_cand.alloc(cap, "hit workspace: candidates");
    d_out.alloc(cap, "hit workspace: verified candidates");
    d_cand_next.alloc(cap, "hit workspace: successors");
    d_cand_status.alloc(cap, "hit workspace: status");
    d_worklist.alloc(cap, "hit workspace: work list");
    hit_cap = cap;
}

void Batch::grow_hit_workspace(uint64_t need) {
    if (getenv("MTSV_TRACE")) fprintf(stderr, "[workspace] seed-hit arrays grow %llu -> %llu entries\n", (unsigned long long)hit_cap, (unsigned long long)need);
    HIP_CHECK(hipStreamSynchronize(stream));
    size_hit_workspace(need);
}

void Batch::VerifyTurn::enter(uint64_t first_read, const Batch* lane) {
    std::unique_lock<std::mutex> lk(mu);
    if (on) {
        const std::pair<uint64_t, const Batch*> me{first_read, lane};
        waiting.push_back(me);
        cv.wait(lk, [&] { return !held && *std::min_element(waiting.begin(), waiting.end()) == me; });
        waiting.erase(std::find(waiting.begin(), waiting.end(), me));
        held = true;
        taken++;
    }
    max_in_verify = std::max(max_in_verify, ++in_verify);
}

void Batch::VerifyTurn::leave() {
    {
        std::lock_guard<std::mutex> lk(mu);
        in_verify--;
        held = false;
    }
    cv.notify_all();
}

void Batch::VerifyTurn::note_grid(uint32_t blocks) {
    std::lock_guard<std::mutex> lk(mu);
    myers_grid_max = std::max<uint64_t>(myers_grid_max, blocks);
}

void Batch::upload(const uint8_t* bases, const uint64_t* read_off, uint64_t n) {
    if (n > max_reads) throw std::runtime_error("arg: batch holds more reads than the workspace was created for");
    const uint64_t first = n ? read_off[0] : 0;
    const uint64_t nb = n ? read_off[n] - first : 0;
    if (nb > max_bases) throw std::runtime_error("arg: batch holds more bases than the workspace was created for");
    h_read_off.resize(n + 1);
    max_len = 0;
    for (uint64_t i = 0; i <= n; i++) {
        if (i && read_off[i] < read_off[i - 1]) throw std::runtime_error("arg: read_off is not ascending");
        h_read_off[i] = (uint32_t)(read_off[i] - first);
        if (i) max_len = std::max(max_len, h_read_off[i] - h_read_off[i - 1]);
    }
    if (n == 0) h_read_off[0] = 0;
    HIP_CHECK(hipSetDevice(di->device));
    if (nb) HIP_CHECK(hipMemcpyAsync(d_bases.p, bases + first, nb, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_read_off.p, h_read_off.data(), (n + 1) * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    n_reads = n;
    n_hits_total = 0;
    total_hits = 0;
    segments.clear();
    last_run = kRunNone;  // (the flags of the run before are not this batch's)
    resident = true;
    codes_resident = mapped = false;
}

void Batch::reset_lane() {
    HIP_CHECK(hipSetDevice(di->device));
    memset(&stats, 0, sizeof stats);
    memset(stage_acc, 0, sizeof stage_acc);
    sw_ms_acc = 0;
    sweep_ms_acc = diag_ms_acc = bound_ms_acc = edit_ms_acc = 0;
    sw_passed_acc = 0;
    n_hits_total = 0;
    n_assign_total = 0;
    if (!hit_cap) size_hit_workspace(hit_cap_first);  // (a growth failed in the run before)
    HIP_CHECK(hipMemsetAsync(d_counters.p, 0, kCounters * sizeof(uint64_t), stream));
    listed_zero = true;
    HIP_CHECK(hipEventRecord(ev[kEvRunBegin], stream));
}

void Batch::finish_lane() {
    HIP_CHECK(hipEventRecord(ev[kEvRunEnd], stream));
    launch_publish(stream, d_counters.p, h_counters.p, kCounters);
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipEventElapsedTime(&stage_acc[7], ev[kEvRunBegin], ev[kEvRunEnd]));
    if (getenv("MTSV_TRACE")) fprintf(stderr, "[lane] last pass: %llu strands of 13..64 seed hits (or more than 4 candidates) to k_coalesce_mid, %llu heavier ones\n",
                                      (unsigned long long)(h_counters.p[kCtrMidStrands] & 0xffffffffull), (unsigned long long)(h_counters.p[kCtrWorklist] >> 32));
    if (getenv("MTSV_TRACE")) fprintf(stderr, "[lane] k_coalesce_heavy: %llu strands walked by runs, %llu by the wavefront walk (a run too long)\n",
                                      (unsigned long long)(h_counters.p[kCtrHeavyWalk] & 0xffffffffull), (unsigned long long)(h_counters.p[kCtrHeavyWalk] >> 32));
    stats.sw_cell_pairs = h_counters.p[kCtrSwCellPairs];
    stats.sw_prefilter_ms = sw_ms_acc;
    stats.sw_sweep_ms = sweep_ms_acc;
    stats.sw_diag_ms = diag_ms_acc;
    stats.sw_bound_ms = bound_ms_acc;
    stats.edit_ms = edit_ms_acc;
    stats.myers_columns = h_counters.p[kCtrMyersColumns];
    stats.n_sw_bound_refuted = h_counters.p[kCtrBoundRefuted];
    stats.n_sw_passed = sw_passed_acc + h_counters.p[kCtrListPassed];  // (+ the successors k_edit_myers' list mode passed by its own bound)
    stats.lf_steps = h_counters.p[kCtrLfSteps];
    stats.n_candidates = h_counters.p[kCtrCandidates];
    stats.n_verified = h_counters.p[kCtrVerified];
    stats.window_bytes = h_counters.p[kCtrWindowBytes];
}

void Batch::begin_run(const mtsv_params& p, uint64_t read_base) {
    if (!(p.edit_rate >= 0.0 && p.edit_rate <= 1.0)) throw std::runtime_error("arg: edit_rate must be within [0, 1]");
    if (!(p.min_seed >= 0.0) || !std::isfinite(p.min_seed)) throw std::runtime_error("arg: min_seed must be finite and >= 0");
    if (p.seed_size == 0 || p.seed_interval == 0) throw std::runtime_error("arg: seed_size and seed_interval must be > 0");
    segments.clear();
    total_hits = 0;
    lanes_used = 1;
    hits_stage.valid = false;
    assign_stage.valid = false;
    assign_stage.staged = 0;
    host_hits_dropped = false;
    last_run = kRunNone;  // until this one completes
    run_t0 = now_s();
    {
        std::lock_guard<std::mutex> lk(verify_turn.mu);
        verify_turn.taken = verify_turn.max_in_verify = verify_turn.myers_grid_max = 0;
    }
    reset_lane();
    for (auto& l : extra) {
        l->verify_mode = verify_mode;
        l->sw_pairs = sw_pairs;
        l->sw_diag = sw_diag;
        l->sw_prepass = sw_prepass;
        l->sw_top = sw_top;
        l->sw_bound = sw_bound;
        l->sw_fused = sw_fused;
        l->reset_lane();
    }
    if (match.mode != MTSV_MATCH_OFF) match_begin(n_reads, read_base);
    if (assign.mode != MTSV_ASSIGN_OFF) collapse_begin();
}

// this run's flags: all zero before any lane's first pass (the lanes' streams do not wait for this one by themselves)
void Batch::match_begin(uint64_t n, uint64_t read_base) {
    const uint64_t need = (n + 63) / 64;
    if (need > match.cap_words() || !match.d_words.p) match.d_words.renew(need + need / 16 + 1, "the match flags");
    match.n_reads = n;
    match.call_base = read_base;
    match.ms = 0;
    match.launches = 0;
    // (the counter sits behind the last word the allocation holds, wherever this run's flags end)
    HIP_CHECK(hipMemsetAsync(match.d_words.p, 0, (match.cap_words() + 1) * sizeof(uint64_t), stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

void Batch::end_run() {
    finish_lane();
    for (auto& l : extra) l->finish_lane();
    const double wall_ms = (now_s() - run_t0) * 1e3;
    // stage times are summed over the lanes (device time per stage); the total is the wall time of the
    // run when lanes overlapped, the stream's own event span otherwise
    bool overlapped = false;
    for (auto& l : extra) {
        if (l->stats.n_passes == 0) continue;
        overlapped = true;
        for (int s = 0; s < 7; s++) stage_acc[s] += l->stage_acc[s];
        stats.n_seed_slots += l->stats.n_seed_slots;
        stats.n_seed_hits += l->stats.n_seed_hits;
        stats.n_passes += l->stats.n_passes;
        stats.n_seed_tile_passes += l->stats.n_seed_tile_passes;
        stats.n_rounds = std::max(stats.n_rounds, l->stats.n_rounds);
        stats.lf_steps += l->stats.lf_steps;
        stats.n_candidates += l->stats.n_candidates;
        stats.n_verified += l->stats.n_verified;
        stats.window_bytes += l->stats.window_bytes;
        stats.sw_cell_pairs += l->stats.sw_cell_pairs;
        stats.sw_prefilter_ms += l->stats.sw_prefilter_ms;
        stats.sw_sweep_ms += l->stats.sw_sweep_ms;
        stats.sw_diag_ms += l->stats.sw_diag_ms;
        stats.sw_bound_ms += l->stats.sw_bound_ms;
        stats.edit_ms += l->stats.edit_ms;
        stats.myers_columns += l->stats.myers_columns;
        stats.n_sw_bound_refuted += l->stats.n_sw_bound_refuted;
        stats.n_sw_passed += l->stats.n_sw_passed;
    }
    if (overlapped) stage_acc[7] = (float)wall_ms;
    for (int s = 0; s < MTSV_N_STAGES; s++) stats.stage_ms[s] = stage_acc[s];
    stats.n_reads = n_reads;
    stats.n_lanes = lanes_used;
    stats.verify_turns = verify_turn.taken;
    stats.verify_lanes_max = verify_turn.max_in_verify;
    stats.myers_grid_max = verify_turn.myers_grid_max;
    total_hits = 0;
    for (auto& sg : segments) total_hits += sg.count;
    stats.n_hits = total_hits;
    if (assign.mode != MTSV_ASSIGN_OFF && assign.trace) collapse_trace("run");
}

// The report's device side: the sorted list of the index's distinct TaxIDs (indexes from the builders are in TaxID
// order; a loaded file is not checked for it, so the host copy of the bins is sorted here) and the counters.
void Batch::set_taxa_report(bool on) {
    if (parent) throw std::runtime_error("internal: the taxa report belongs to the workspace's owner");
    if (on && match.mode == MTSV_MATCH_ONLY)
        throw std::runtime_error("arg: the taxa report reads gathered hits and MTSV_MATCH_ONLY gathers none (mtsv_batch_set_match_flags)");
    if (on && !report.d_counts.p) {
        std::vector<uint32_t>& t = report.h_taxa;
        t.clear();
        for (const Bin& b : ix->host.bins) t.push_back(b.tax_id);
        std::sort(t.begin(), t.end());
        t.erase(std::unique(t.begin(), t.end()), t.end());
        if (t.size() >= (1ull << 30)) throw std::runtime_error("limit: taxa report of 2^30 TaxIDs or more");
        report.n_taxa = (uint32_t)t.size();
        uint32_t dense_max = kReportDenseTaxa;
        if (const char* e = getenv("MTSV_REPORT_DENSE_MAX")) dense_max = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), kReportDenseTaxa);  // (tests)
        report.dense = report.n_taxa <= dense_max;
        if (const char* e = getenv("MTSV_REPORT_HASH_SLOTS")) {  // (tests: a table small enough to overflow)
            const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 16), kReportHashSlots);
            report.hash_slots = 16;
            while (report.hash_slots * 2 <= want) report.hash_slots *= 2;
        }
        report.trace = getenv("MTSV_TRACE") != nullptr;
        if (report.trace)
            fprintf(stderr, "[report] %u taxa: %s tier (dense up to %u taxa, hash table of %u slots)\n", report.n_taxa,
                    report.dense ? "dense" : "hashed", dense_max, report.hash_slots);
        HIP_CHECK(hipSetDevice(di->device));
        report.d_taxa.alloc(report.n_taxa, "the report's TaxIDs");
        report.d_counts.alloc(4ull * report.n_taxa + 2, "the report's counters");
        if (report.n_taxa) HIP_CHECK(hipMemcpyAsync(report.d_taxa.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemsetAsync(report.d_counts.p, 0, (4ull * report.n_taxa + 2) * 8, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    report.on = on;
}

void Batch::taxa_report(std::vector<mtsv_taxon_stats>& rows, uint64_t* total_reads, float* device_ms, bool reset) {
    if (!report.on) throw std::runtime_error("arg: the taxa report of this workspace is not switched on (mtsv_batch_set_taxa_report)");
    HIP_CHECK(hipSetDevice(di->device));
    const uint64_t n = 4ull * report.n_taxa + 2;
    std::vector<uint64_t> c(n);
    // (every run is synchronous: no lane has a pass in flight)
    HIP_CHECK(hipMemcpyAsync(c.data(), report.d_counts.p, n * 8, hipMemcpyDeviceToHost, stream));
    if (reset) HIP_CHECK(hipMemsetAsync(report.d_counts.p, 0, n * 8, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    rows.clear();
    for (uint32_t k = 0; k < report.n_taxa; k++) {
        const uint64_t* q = &c[4ull * k];
        if (q[0] | q[1] | q[2] | q[3]) rows.push_back(mtsv_taxon_stats{report.h_taxa[k], 0, q[0], q[1], q[2], q[3]});
    }
    *total_reads = c[n - 2];
    std::lock_guard<std::mutex> lk(report.mu);
    *device_ms = report.ms;
    if (report.trace)
        fprintf(stderr, "[report] %llu kernel launches, %.3f ms, %llu atomic adds on the global counters\n", (unsigned long long)report.launches,
                report.ms, (unsigned long long)c[n - 1]);
    if (reset) report.ms = 0, report.launches = 0;
}

void Batch::set_match_flags(int mode) {
    if (parent) throw std::runtime_error("internal: the match flags belong to the workspace's owner");
    if (mode != MTSV_MATCH_OFF && mode != MTSV_MATCH_WITH_HITS && mode != MTSV_MATCH_ONLY) throw std::runtime_error("arg: bad match-flags mode");
    if (mode == MTSV_MATCH_ONLY && report.on)
        throw std::runtime_error("arg: MTSV_MATCH_ONLY gathers no hits and the taxa report of this workspace, which reads them, is on");
    if (mode == MTSV_MATCH_ONLY && assign.mode != MTSV_ASSIGN_OFF)
        throw std::runtime_error("arg: MTSV_MATCH_ONLY gathers no hits and the assignments of this workspace, which are reduced from them, are on");
    if (mode != MTSV_MATCH_OFF && match.mode == MTSV_MATCH_OFF) match.n_reads = 0;  // no run to speak of yet
    match.trace = getenv("MTSV_TRACE") != nullptr;
    match.mode = mode;
}

void Batch::match_flags(std::vector<uint64_t>& words, uint64_t* n_reads_out, uint64_t* n_matched) {
    if (match.mode == MTSV_MATCH_OFF) throw std::runtime_error("arg: the match flags of this workspace are not switched on (mtsv_batch_set_match_flags)");
    const uint64_t nw = (match.n_reads + 63) / 64;
    words.assign(std::max<uint64_t>(nw, 1), 0);
    *n_reads_out = match.n_reads;
    *n_matched = 0;
    if (!match.n_reads) return;
    HIP_CHECK(hipSetDevice(di->device));
    // (every run is synchronous: no lane has a pass in flight)
    HIP_CHECK(hipMemcpyAsync(words.data(), match.d_words.p, nw * 8, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(n_matched, match.d_words.p + match.cap_words(), 8, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    std::lock_guard<std::mutex> lk(match.mu);
    if (match.trace)
        fprintf(stderr, "[match] %llu kernel launches, %.3f ms, %llu of %llu reads matched, %llu bytes of flags to the host\n",
                (unsigned long long)match.launches, match.ms, (unsigned long long)*n_matched, (unsigned long long)match.n_reads,
                (unsigned long long)(nw * 8 + 8));
}

// ---- assignments (k_collapse.hip) ----
void Batch::set_assignments(int mode) {
    if (parent) throw std::runtime_error("internal: the assignments belong to the workspace's owner");
    if (mode != MTSV_ASSIGN_OFF && mode != MTSV_ASSIGN_WITH_HITS && mode != MTSV_ASSIGN_ONLY) throw std::runtime_error("arg: bad assignments mode");
    if (mode != MTSV_ASSIGN_OFF && match.mode == MTSV_MATCH_ONLY)
        throw std::runtime_error("arg: assignments are reduced from gathered hits and MTSV_MATCH_ONLY gathers none (mtsv_batch_set_match_flags)");
    if (mode != MTSV_ASSIGN_OFF && assign.mode == MTSV_ASSIGN_OFF) {
        for (auto& sg : segments) sg.a_offset = sg.a_count = 0;  // no run to speak of yet
        // the tier edges (tests move them to reach every tier with small databases)
        auto env_u = [](const char* name, uint32_t dflt, uint32_t lo, uint32_t hi) {
            const char* e = getenv(name);
            if (!e) return dflt;
            const long long v = atoll(e);
            return (uint32_t)std::max<long long>(lo, std::min<long long>(hi, v));
        };
        assign.lane_max = env_u("MTSV_COLLAPSE_LANE_MAX", kCollapseLaneMax, 1, kCollapseLaneMax);
        assign.wave_max = env_u("MTSV_COLLAPSE_WAVE_MAX", 64, 1, 64);
        // (a 16-byte key halves what the 32 KiB of the LDS tier hold)
        const uint32_t lds_keys = assign.grain == MTSV_GRAIN_TAXID ? kCollapseLdsKeys : kCollapseLdsKeysWide;
        uint32_t lds = env_u("MTSV_COLLAPSE_LDS_MAX", lds_keys, 2, lds_keys);
        while (lds & (lds - 1)) lds &= lds - 1;  // (a power of two: the largest one not above what was asked for)
        assign.lds_max = lds;
        assign.trace = getenv("MTSV_TRACE") != nullptr;
        assign.ms = 0;
        assign.launches = 0;
        for (auto& t : assign.tiers) t = 0;
    }
    assign.mode = mode;
}

void Batch::set_assignment_grain(int grain) {
    if (parent) throw std::runtime_error("internal: the assignments belong to the workspace's owner");
    if (grain != MTSV_GRAIN_TAXID && grain != MTSV_GRAIN_TAXID_GI && grain != MTSV_GRAIN_LONG) throw std::runtime_error("arg: bad assignment grain");
    if (assign.mode != MTSV_ASSIGN_OFF)
        throw std::runtime_error("arg: the grain changes only while the assignments are off (mtsv_batch_set_assignments): the record arrays hold one record size");
    if (grain == assign.grain) return;
    assign.grain = grain;
    // the pinned array a host batch left was sized in the old records
    assign_stage.drop();
    assign_stage.rec = assign.rec_bytes();
    assign_stage.last_total = 0;
}

void Batch::collapse_begin() {
    std::lock_guard<std::mutex> lk(assign.mu);
    assign.ms = 0;
    assign.launches = 0;
    for (auto& t : assign.tiers) t = 0;
}

void Batch::collapse_trace(const char* what) {
    uint64_t n_a = 0, n_h = 0;
    for (auto& sg : segments) n_a += sg.a_count, n_h += sg.count;
    std::lock_guard<std::mutex> lk(assign.mu);
    fprintf(stderr, "[collapse] %s: %llu launches, %.3f ms, %llu hits -> %llu assignments; reads by tier: lane %llu, wavefront %llu, lds %llu, global %llu "
                    "(tiers end at %u / %u / %u hits)%s\n",
            what, (unsigned long long)assign.launches, assign.ms, (unsigned long long)n_h, (unsigned long long)n_a, (unsigned long long)assign.tiers[0],
            (unsigned long long)assign.tiers[1], (unsigned long long)assign.tiers[3], (unsigned long long)assign.tiers[4], assign.lane_max, assign.wave_max,
            assign.lds_max, assign.grain == MTSV_GRAIN_LONG ? " [grain long]" : assign.grain == MTSV_GRAIN_TAXID_GI ? " [grain taxid-gi]" : "");
}

void Batch::collapse_room(uint64_t n_pass_reads, uint64_t n_hits) {
    CollapseScratch& c = collapse;
    const Assignments& as = root()->assign;
    const uint64_t rec = as.rec_bytes(), key_bytes = as.key_bytes();
    if (n_hits >= (1ull << 32)) throw std::runtime_error("limit: 2^32 hits or more in one pass of the collapse");
    if (!c.d_ctr.p) c.d_ctr.alloc(kCollapseCounters, "the collapse counters");
    if (!c.h_ctr.p) c.h_ctr.renew(kCollapseCounters, hipHostMallocMapped);
    c.ev.create();
    if (n_hits > c.cap_hits || !c.cap_hits || c.key_bytes != key_bytes) {
        HIP_CHECK(hipStreamSynchronize(stream));
        c.resize(std::min<uint64_t>(std::max<uint64_t>(n_hits + n_hits / 8, 1ull << 16), 0xffffffffull), key_bytes);
    }
    if (n_pass_reads > c.list.cap || !c.list.p) {
        HIP_CHECK(hipStreamSynchronize(stream));
        c.list.renew(std::max<uint64_t>(n_pass_reads + n_pass_reads / 16, 1024), "collapse scratch: read list");
    }
    if ((n_assign_total + n_hits) * rec > d_assign.cap || !d_assign.p) {
        // grow the result array, keeping what earlier passes produced (a failure leaves the lane as it was; the old array
        // leaves with this one)
        DevBuf<uint8_t> grown;
        grown.alloc(std::max<uint64_t>(std::max(d_assign.cap * 2, (n_assign_total + n_hits) * rec), (1ull << 16) * rec), "the assignments");
        if (n_assign_total) HIP_CHECK(hipMemcpyAsync(grown.p, d_assign.p, n_assign_total * rec, hipMemcpyDeviceToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        // run_host may be copying an earlier range's assignments out of the old array on the owner's copy stream (and another
        // lane's thread may be issuing such a copy right now: the commit mutex covers the pointer swap), as with d_hits
        std::unique_lock<std::mutex> commit_lk;
        if (root()->commit_mu) commit_lk = std::unique_lock<std::mutex>(*root()->commit_mu);
        if (root()->commit_mu && root()->copy_stream2) HIP_CHECK(hipStreamSynchronize(root()->copy_stream2));
        d_assign.swap(grown);
    }
}

void Batch::CollapseScratch::resize(uint64_t hits, uint64_t kb) {
    cap_hits = 0;
    release_all(keys, flags, place, tiles);
    keys.alloc(hits * (kb / 8), "collapse scratch: keys");
    key_bytes = kb;
    flags.alloc(hits + 1, "collapse scratch: flags");
    place.alloc(hits + 1, "collapse scratch: places");
    tiles.alloc((uint64_t)scan_tiles((uint32_t)hits) + 1, "collapse scratch: tile sums");
    cap_hits = hits;
}

void Batch::collapse_enqueue(uint32_t n_pass_reads, const uint32_t* strand_nout, const uint32_t* out_off, const DevHit* hits, uint64_t n_hits) {
    const Assignments& as = root()->assign;
    collapse_room(n_pass_reads, n_hits);
    CollapseScratch& c = collapse;
    c.pending_hits = n_hits;
    HIP_CHECK(hipEventRecord(c.ev[0], stream));
    launch_collapse(stream, as.grain, n_pass_reads, strand_nout, out_off, hits, (uint32_t)n_hits, as.lane_max, as.wave_max, as.lds_max, c.keys.p, c.flags.p,
                    c.place.p, c.tiles.p, c.list.p, c.d_ctr.p, d_assign.p + n_assign_total * as.rec_bytes());
    HIP_CHECK(hipEventRecord(c.ev[1], stream));
    // the pass's record count reaches the host with the synchronise the pass ends with anyway
    launch_publish(stream, c.d_ctr.p, c.h_ctr.p, kCollapseCounters);
}

uint64_t Batch::collapse_commit() {
    Assignments& as = root()->assign;
    CollapseScratch& c = collapse;
    const uint64_t cnt = c.h_ctr.p[kCollapseCtrTotal];
    if (cnt > c.pending_hits) throw std::runtime_error("internal: the collapse wrote " + std::to_string(cnt) + " assignments from " + std::to_string(c.pending_hits) + " hits");
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    n_assign_total += cnt;
    std::lock_guard<std::mutex> lk(as.mu);
    as.ms += ms;
    as.launches++;
    for (int t = 0; t < 5; t++) as.tiers[t] += c.h_ctr.p[kCollapseCtrLane + t];
    return cnt;
}

void Batch::download_assignments(void** a, uint64_t* n, float* device_ms, bool wide) {
    if (parent) throw std::runtime_error("internal: the assignments belong to the workspace's owner");
    if (assign.mode == MTSV_ASSIGN_OFF) throw std::runtime_error("arg: the assignments of this workspace are not switched on (mtsv_batch_set_assignments)");
    if (wide != (assign.grain != MTSV_GRAIN_TAXID))
        throw std::runtime_error(wide ? "arg: the grain of this workspace is MTSV_GRAIN_TAXID: its records are mtsv_assignment (mtsv_batch_download_assignments)"
                                      : "arg: the grain of this workspace is not MTSV_GRAIN_TAXID: its records are mtsv_assignment_gi (mtsv_batch_download_assignments_gi)");
    const uint64_t rec = assign.rec_bytes();
    HIP_CHECK(hipSetDevice(di->device));
    uint64_t total = 0;
    for (auto& sg : segments) total += sg.a_count;
    assign_stage.last_total = total;
    uint8_t* out = nullptr;
    if (assign_stage.valid && assign_stage.p && assign_stage.staged == total) {  // run_host already brought them over
        out = (uint8_t*)assign_stage.hand_out();
    } else {
        uint64_t cap = 0;
        out = (uint8_t*)pinned_hits_alloc((total * rec + 31) / 32, &cap);  // (the pool counts in 32-byte hits)
        uint64_t at = 0;
        // (every run is synchronous: no lane has a pass in flight)
        for (auto& sg : segments) {
            if (!sg.a_count) continue;
            const hipError_t e = hipMemcpy(out + at * rec, sg.lane->d_assign.p + sg.a_offset * rec, sg.a_count * rec, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                pinned_hits_release(out);
                throw_hip(e, "hipMemcpy(assignments)", __FILE__, __LINE__);
            }
            at += sg.a_count;
        }
    }
    *a = out;
    *n = total;
    std::lock_guard<std::mutex> lk(assign.mu);
    if (device_ms) *device_ms = assign.ms;
}

void Batch::run(const mtsv_params& p) {
    begin_run(p);
    // (a batch take_reads left is codes already: fast_code would turn every one of them into N)
    run_range(p, codes_resident ? nullptr : d_bases.p, d_codes.p, d_read_off.p, h_read_off.data(), n_reads, max_len, 0);
    end_run();
    last_run = kRunResident;
}

// d_compact for `tiles` tiles of the compaction kernels, and d_read_map (take_reads, and DupMap::take_unique of dedup.hip)
void Batch::compact_room(uint64_t tiles) {
    if (!d_compact.p || compact_cap() < tiles) d_compact.renew(3 + 2 * (tiles + tiles / 16), "the compaction's tile sums");
    if (!d_read_map.p) d_read_map.alloc(max_reads, "the read map");
}

// ---------------------------------------------------------------------------------------------
// Chaining: the unmatched (matched) reads of src's last run become this workspace's resident batch.  The bases go from
// HBM to HBM, the flags are read where k_match wrote them; the host sees the 24-byte result block (the capacity check
// needs the counts before anything is written) and the survivors' offsets, which run_range cuts its chunks by.
// ---------------------------------------------------------------------------------------------
void Batch::take_reads(Batch& src, int keep, uint64_t* n_kept, uint64_t* bases_kept, float* device_ms) {
    if (parent || src.parent) throw std::runtime_error("internal: take_reads on a lane");
    if (&src == this) throw std::runtime_error("arg: take_reads from a workspace into itself");
    if (keep != MTSV_KEEP_UNMATCHED && keep != MTSV_KEEP_MATCHED) throw std::runtime_error("arg: bad keep (MTSV_KEEP_UNMATCHED or MTSV_KEEP_MATCHED)");
    if (src.di->device != di->device) throw std::runtime_error("arg: take_reads between workspaces of different devices");
    if (src.match.mode == MTSV_MATCH_OFF) throw std::runtime_error("arg: the match flags of the source workspace are not switched on (mtsv_batch_set_match_flags)");
    if (src.last_run == kRunHostSegments)
        throw std::runtime_error("arg: the source's host batch took turns through the input segments: its first reads are no longer in HBM");
    if (src.last_run == kRunMerged) throw std::runtime_error("arg: the source workspace holds a merge of other workspaces' runs (mtsv_batch_merge_runs): its flags describe reads it does not hold");
    if (src.last_run == kRunNone) throw std::runtime_error("arg: the source workspace has no completed run whose reads are still in HBM");
    // (flags switched on after the last run: they describe no run yet)
    if (src.match.n_reads != src.n_reads) throw std::runtime_error("arg: the source workspace has no completed run since its match flags were switched on");
    const bool trace = getenv("MTSV_TRACE") != nullptr;
    const uint64_t n = src.n_reads;
    const bool host_batch = src.last_run == kRunHostOneSegment;
    const uint8_t* s_codes = host_batch ? src.arena[0].d_bases.p : src.d_codes.p;
    const uint32_t* s_off = host_batch ? src.arena[0].d_off.p : src.d_read_off.p;
    const uint32_t* s_map = src.mapped ? src.d_read_map.p : nullptr;
    HIP_CHECK(hipSetDevice(di->device));
    compact_room(compact_tiles(n));
    if (!compact_ev.created()) compact_ev.create();
    uint64_t* result = d_compact.p;
    uint64_t *tile_cnt = d_compact.p + 3, *tile_bases = d_compact.p + 3 + compact_cap();
    HIP_CHECK(hipMemsetAsync(result, 0, 3 * sizeof(uint64_t), stream));
    HIP_CHECK(hipEventRecord(compact_ev[0], stream));
    launch_compact_scan(stream, (uint32_t)n, src.match.d_words.p, s_off, keep, tile_cnt, tile_bases, result);
    HIP_CHECK(hipEventRecord(compact_ev[1], stream));
    uint64_t h_result[3] = {0, 0, 0};
    HIP_CHECK(hipMemcpyAsync(h_result, result, sizeof h_result, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    const uint64_t m = h_result[0], nb = h_result[1];
    if (m > max_reads || nb > max_bases)
        throw std::runtime_error("arg: " + std::to_string(m) + " reads of " + std::to_string(nb) + " bases survive, the destination workspace was created for " +
                                 std::to_string(max_reads) + " reads of " + std::to_string(max_bases) + " bases");
    // from here on the destination's resident batch is being replaced
    resident = false;
    last_run = kRunNone;
    HIP_CHECK(hipEventRecord(compact_ev[2], stream));
    launch_compact_copy(stream, (uint32_t)n, src.match.d_words.p, s_off, s_codes, keep, s_map, tile_cnt, tile_bases, result, d_codes.p, d_read_off.p, d_read_map.p);
    HIP_CHECK(hipEventRecord(compact_ev[3], stream));
    h_read_off.resize(m + 1);
    HIP_CHECK(hipMemcpyAsync(h_read_off.data(), d_read_off.p, (m + 1) * 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (h_read_off[0] != 0 || h_read_off[m] != nb) throw std::runtime_error("internal: offsets of the compacted batch do not close on its bases");
    float ms_scan = 0, ms_copy = 0;
    HIP_CHECK(hipEventElapsedTime(&ms_scan, compact_ev[0], compact_ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms_copy, compact_ev[2], compact_ev[3]));
    n_reads = m;
    max_len = (uint32_t)h_result[2];
    n_hits_total = 0;
    total_hits = 0;
    segments.clear();
    resident = codes_resident = mapped = true;
    *n_kept = m;
    *bases_kept = nb;
    if (device_ms) *device_ms = ms_scan + ms_copy;
    if (trace)
        fprintf(stderr, "[compact] %llu of %llu reads kept (%s), %llu bases; scan %.3f ms, copy %.3f ms; %llu bytes to the host, 0 to the device\n",
                (unsigned long long)m, (unsigned long long)n, keep == MTSV_KEEP_MATCHED ? "matched" : "unmatched", (unsigned long long)nb, ms_scan, ms_copy,
                (unsigned long long)(sizeof h_result + (m + 1) * 4));
}

// ---------------------------------------------------------------------------------------------
// The resident batch of another workspace of the device, copied: what several chunks of a database need of the same reads
// (one upload, or one take_reads behind a filter, and a copy per further chunk).  Plain device-to-device copies; the host
// copies its offset table.
// ---------------------------------------------------------------------------------------------
void Batch::copy_reads(Batch& src, float* device_ms) {
    if (parent || src.parent) throw std::runtime_error("internal: copy_reads on a lane");
    if (&src == this) throw std::runtime_error("arg: copy_reads from a workspace into itself");
    if (src.di->device != di->device) throw std::runtime_error("arg: copy_reads between workspaces of different devices");
    const bool host_batch = !src.resident && src.last_run == kRunHostOneSegment;
    if (!src.resident && !host_batch)
        throw std::runtime_error("arg: the source workspace holds no resident batch (mtsv_batch_upload, mtsv_batch_take_reads, mtsv_batch_copy_reads, or a host batch of one input segment)");
    const uint64_t n = src.n_reads;
    const uint32_t* ho = host_batch ? src.h_off_all.p : src.h_read_off.data();
    const uint64_t nb = n ? ho[n] : 0;
    if (n > max_reads || nb > max_bases)
        throw std::runtime_error("arg: the source holds " + std::to_string(n) + " reads of " + std::to_string(nb) + " bases, the destination workspace was created for " +
                                 std::to_string(max_reads) + " reads of " + std::to_string(max_bases) + " bases");
    const bool codes = host_batch || src.codes_resident;
    const bool with_map = !host_batch && src.mapped;
    const uint8_t* s_bytes = host_batch ? src.arena[0].d_bases.p : codes ? src.d_codes.p : src.d_bases.p;
    const uint32_t* s_off = host_batch ? src.arena[0].d_off.p : src.d_read_off.p;
    HIP_CHECK(hipSetDevice(di->device));
    if (with_map && !d_read_map.p) d_read_map.alloc(max_reads, "the read map");
    if (!compact_ev.created()) compact_ev.create();
    // from here on the destination's resident batch is being replaced
    resident = false;
    last_run = kRunNone;
    HIP_CHECK(hipEventRecord(compact_ev[0], stream));
    if (nb) HIP_CHECK(hipMemcpyDtoDAsync(codes ? d_codes.p : d_bases.p, const_cast<uint8_t*>(s_bytes), nb, stream));
    if (n) HIP_CHECK(hipMemcpyDtoDAsync(d_read_off.p, const_cast<uint32_t*>(s_off), (n + 1) * 4, stream));
    else HIP_CHECK(hipMemsetAsync(d_read_off.p, 0, 4, stream));
    if (with_map && n) HIP_CHECK(hipMemcpyDtoDAsync(d_read_map.p, src.d_read_map.p, n * 4, stream));
    HIP_CHECK(hipEventRecord(compact_ev[1], stream));
    if (n) h_read_off.assign(ho, ho + n + 1);
    else h_read_off.assign(1, 0u);
    HIP_CHECK(hipStreamSynchronize(stream));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, compact_ev[0], compact_ev[1]));
    n_reads = n;
    max_len = src.max_len;
    n_hits_total = 0;
    total_hits = 0;
    segments.clear();
    resident = true;
    codes_resident = codes;
    mapped = with_map;
    if (device_ms) *device_ms = ms;
    if (getenv("MTSV_TRACE"))
        fprintf(stderr, "[copy_reads] %llu reads, %llu bases (%s%s), %.3f ms; 0 bytes to the host, 0 to the device\n", (unsigned long long)n, (unsigned long long)nb,
                codes ? "codes" : "bases as uploaded", with_map ? ", mapped" : "", ms);
}

// ---------------------------------------------------------------------------------------------
// Merging the runs of several workspaces over the same reads (the chunks of one database): k_merge.hip puts the hits
// together per read in this workspace's result array, laid out as one pass, so that the report and the flags take the
// merged reads with the kernels a pass uses and download() returns the list.  Everything the merge needs to know of the
// sources is on the host (counts, segments, offsets); the host reads back the scan's total and the copy's count of hits without a place, 16 bytes.
// ---------------------------------------------------------------------------------------------
void Batch::report_extend(Batch* const* srcs, int n_srcs) {
    // (checked on every merge, from the sources' indexes as they are now: nothing is remembered about an index handle)
    std::vector<uint32_t> u = report.h_taxa;
    for (int k = 0; k < n_srcs; k++) {
        if (srcs[k]->ix == ix) continue;  // (the list began as this index's)
        std::vector<uint32_t> t;
        for (const Bin& b : srcs[k]->ix->host.bins) t.push_back(b.tax_id);
        std::sort(t.begin(), t.end());
        t.erase(std::unique(t.begin(), t.end()), t.end());
        u.insert(u.end(), t.begin(), t.end());
    }
    std::sort(u.begin(), u.end());
    u.erase(std::unique(u.begin(), u.end()), u.end());
    if (u.size() >= (1ull << 30)) throw std::runtime_error("limit: taxa report of 2^30 TaxIDs or more");
    if (u.size() == report.h_taxa.size()) return;  // (a superset of the same size: nothing new)
    // new TaxIDs: the list and the counters so far, rebuilt (host work; a database's chunks bring theirs once)
    const uint64_t n_old = 4ull * report.n_taxa + 2, n_new = 4ull * u.size() + 2;
    std::vector<uint64_t> c_old(n_old), c_new(n_new, 0);
    HIP_CHECK(hipMemcpyAsync(c_old.data(), report.d_counts.p, n_old * 8, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (uint32_t k = 0; k < report.n_taxa; k++) {
        const uint64_t at = (uint64_t)(std::lower_bound(u.begin(), u.end(), report.h_taxa[k]) - u.begin());
        for (int q = 0; q < 4; q++) c_new[4 * at + q] = c_old[4ull * k + q];
    }
    c_new[n_new - 2] = c_old[n_old - 2];
    c_new[n_new - 1] = c_old[n_old - 1];
    DevBuf<uint32_t> nt;  // (the old arrays leave with these)
    DevBuf<uint64_t> nc;
    nt.alloc(u.size(), "the report's TaxIDs");
    nc.alloc(n_new, "the report's counters");
    HIP_CHECK(hipMemcpyAsync(nt.p, u.data(), u.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(nc.p, c_new.data(), n_new * 8, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    report.d_taxa.swap(nt);
    report.d_counts.swap(nc);
    report.h_taxa.swap(u);
    report.n_taxa = (uint32_t)report.h_taxa.size();
    uint32_t dense_max = kReportDenseTaxa;
    if (const char* e = getenv("MTSV_REPORT_DENSE_MAX")) dense_max = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), kReportDenseTaxa);  // (tests)
    report.dense = report.n_taxa <= dense_max;
    if (report.trace)
        fprintf(stderr, "[report] list rebuilt for a merge: %u taxa, %s tier\n", report.n_taxa, report.dense ? "dense" : "hashed");
}

void Batch::merge_runs(Batch* const* srcs, int n_srcs, float* device_ms) {
    if (parent) throw std::runtime_error("internal: merge_runs on a lane");
    if (n_srcs < 1 || n_srcs > 64) throw std::runtime_error("arg: merge_runs takes 1 to 64 sources");
    if (match.mode == MTSV_MATCH_ONLY) throw std::runtime_error("arg: the destination workspace is in MTSV_MATCH_ONLY, which keeps no hits");
    for (int k = 0; k < n_srcs; k++) {
        const Batch* s = srcs[k];
        if (!s) throw std::runtime_error("arg: null source workspace");
        if (s->parent) throw std::runtime_error("internal: merge_runs from a lane");
        if (s == this) throw std::runtime_error("arg: the destination workspace is among the sources");
        if (s->di->device != di->device) throw std::runtime_error("arg: merge_runs between workspaces of different devices");
        if (s->match.mode == MTSV_MATCH_ONLY) throw std::runtime_error("arg: a source workspace is in MTSV_MATCH_ONLY: its run gathered no hits");
        if (s->last_run == kRunHostOneSegment || s->last_run == kRunHostSegments)
            throw std::runtime_error("arg: a source's last run was a host batch (merge_runs takes runs on a resident batch: mtsv_batch_upload / _take_reads / _copy_reads + mtsv_batch_run)");
        if (s->last_run != kRunResident) throw std::runtime_error("arg: a source workspace has no completed run on a resident batch whose hits are still in HBM");
    }
    const Batch& s0 = *srcs[0];
    const uint64_t n = s0.n_reads;
    uint64_t total = 0;
    std::vector<MergePart> parts;
    uint64_t max_part_reads = 0, max_part_hits = 0;
    for (int k = 0; k < n_srcs; k++) {
        const Batch& s = *srcs[k];
        if (s.n_reads != n) throw std::runtime_error("arg: the sources hold different numbers of reads");
        if (memcmp(s.h_read_off.data(), s0.h_read_off.data(), (n + 1) * sizeof(uint32_t)) != 0)
            throw std::runtime_error("arg: the sources' reads have different offsets: not the same batch");
        if (s.mapped != s0.mapped) throw std::runtime_error("arg: some sources carry a read map and some do not");
        total += s.total_hits;
        uint64_t next = 0;
        for (const Segment& sg : s.segments) {
            if (sg.first_read != next) throw std::runtime_error("internal: a source's segments do not follow each other in read order");
            next += sg.n_reads;
            if (sg.count >= (1ull << 32)) throw std::runtime_error("limit: 2^32 hits or more in one stretch of a source");
            if (!sg.n_reads) continue;
            parts.push_back(MergePart{sg.lane->d_hits.p + sg.offset, (uint32_t)sg.count, (uint32_t)sg.first_read, (uint32_t)sg.n_reads, (uint32_t)k, 0});
            max_part_reads = std::max(max_part_reads, sg.n_reads);
            max_part_hits = std::max(max_part_hits, sg.count);
        }
        if (next != n) throw std::runtime_error("internal: a source's segments do not cover its reads");
    }
    if (total >= (1ull << 32)) throw std::runtime_error("limit: the merge holds " + std::to_string(total) + " hits, 2^32 or more");
    if (parts.size() > 65535) throw std::runtime_error("limit: more than 65535 stretches of hits in the sources of one merge");
    const uint32_t* map = s0.mapped ? s0.d_read_map.p : nullptr;
    HIP_CHECK(hipSetDevice(di->device));
    // ---- room (created by the first merge; whatever fails here leaves the last result where it was) ----
    MergeState& m = merge;
    if (!m.ev.created()) m.ev.create();
    if (n > m.cap_reads || !m.d_nout.p) {
        m.cap_reads = 0;
        release_all(m.d_nout, m.d_off, m.d_tiles);
        const uint64_t cap = std::min<uint64_t>(n + n / 16, 0x7fffffffull);  // (a workspace's limit)
        m.d_nout.alloc(2 * cap + 1, "merge: hit counts");
        m.d_off.alloc(2 * cap + 1, "merge: hit offsets");
        m.d_tiles.alloc((uint64_t)scan_tiles((uint32_t)(2 * cap)) + 1 + 2, "merge: tile sums");
        m.cap_reads = cap;
    }
    if ((uint64_t)n_srcs * n > m.cap_sn || !m.d_lo.p) {
        m.cap_sn = 0;
        release_all(m.d_lo, m.d_base);
        const uint64_t cap = (uint64_t)n_srcs * (n + n / 16);
        m.d_lo.alloc(cap, "merge: lower bounds");
        m.d_base.alloc(cap, "merge: hit bases");
        m.cap_sn = cap;
    }
    if (parts.size() > m.d_parts.cap || !m.d_parts.p) m.d_parts.renew(std::max<uint64_t>(parts.size() * 2, 64), "merge: stretches");
    // (before the result array grows, so that it cannot fail once the result is being replaced; if that allocation then
    //  fails, the list has grown already, with the counts so far kept and the new rows 0: the header says so)
    if (report.on) report_extend(srcs, n_srcs);
    // (the collapse's scratch and the room behind the assignments so far: the last ones stay readable until then)
    if (assign.mode != MTSV_ASSIGN_OFF && n) collapse_room(n, total);
    DevBuf<DevHit> grown;  // (the last result stays in the old array until nothing can refuse the merge any more)
    if (total > d_hits.cap) grown.alloc(total + total / 16, "the result array");
    // ---- from here on the destination's result is being replaced ----
    if (grown.p) {
        d_hits.swap(grown);
        grown.release();
    }
    segments.clear();
    total_hits = 0;
    n_hits_total = 0;
    hits_stage.valid = false;
    assign_stage.valid = false;
    host_hits_dropped = false;
    last_run = kRunNone;
    memset(&stats, 0, sizeof stats);
    if (match.mode != MTSV_MATCH_OFF) match_begin(n, 0);
    const bool collapse_on = assign.mode != MTSV_ASSIGN_OFF;
    n_assign_total = 0;
    if (collapse_on) collapse_begin();
    uint64_t n_assign = 0;
    uint64_t h_total[2] = {0, 0};  // the scan's total, the hits the copy could not place
    float ms = 0, ms_report = 0, ms_match = 0;
    if (n) {
        HIP_CHECK(hipMemcpyAsync(m.d_parts.p, parts.data(), parts.size() * sizeof(MergePart), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemsetAsync(m.d_tiles.p + m.cap_tiles(), 0, 2 * sizeof(uint64_t), stream));
        HIP_CHECK(hipEventRecord(m.ev[0], stream));
        launch_merge_bounds(stream, m.d_parts.p, (uint32_t)parts.size(), (uint32_t)max_part_reads, (uint32_t)n, map, m.d_lo.p, m.d_base.p);
        launch_merge_sum(stream, (uint32_t)n, (uint32_t)n_srcs, m.d_lo.p, m.d_base.p, m.d_nout.p);
        launch_scan(stream, m.d_nout.p, (uint32_t)(2 * n), m.d_tiles.p, m.d_tiles.p + m.cap_tiles(), m.d_off.p);
        launch_merge_copy(stream, m.d_parts.p, (uint32_t)parts.size(), (uint32_t)max_part_hits, (uint32_t)n, map, m.d_base.p, m.d_off.p, d_hits.p, (uint32_t)total, m.d_tiles.p + m.cap_tiles() + 1);
        HIP_CHECK(hipEventRecord(m.ev[1], stream));
        HIP_CHECK(hipMemcpyAsync(h_total, m.d_tiles.p + m.cap_tiles(), sizeof h_total, hipMemcpyDeviceToHost, stream));
        if (report.on) {
            if (!report_ev.created()) report_ev.create();
            HIP_CHECK(hipEventRecord(report_ev[0], stream));
            launch_report(stream, (uint32_t)n, m.d_nout.p, m.d_off.p, d_hits.p, report.d_taxa.p, report.n_taxa, report.dense, report.hash_slots, report.d_counts.p,
                          report.d_counts.p + 4ull * report.n_taxa, report.trace ? report.d_counts.p + 4ull * report.n_taxa + 1 : nullptr);
            HIP_CHECK(hipEventRecord(report_ev[1], stream));
        }
        if (match.mode != MTSV_MATCH_OFF) {
            if (!match_ev.created()) match_ev.create();
            HIP_CHECK(hipEventRecord(match_ev[0], stream));
            launch_match(stream, (uint32_t)n, m.d_nout.p, 0, match.d_words.p, match.d_words.p + match.cap_words());
            HIP_CHECK(hipEventRecord(match_ev[1], stream));
        }
        // the collector is laid out as one pass: its assignments are those of the merged reads, all sources together
        if (collapse_on) collapse_enqueue((uint32_t)n, m.d_nout.p, m.d_off.p, d_hits.p, total);
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        if (collapse_on) n_assign = collapse_commit();
        if (h_total[0] != total)
            throw std::runtime_error("internal: the merge counted " + std::to_string(h_total[0]) + " hits, the sources hold " + std::to_string(total));
        if (h_total[1])
            throw std::runtime_error("internal: " + std::to_string(h_total[1]) + " hits of the sources have no place in the merge: a source's hits are not ordered by read");
        HIP_CHECK(hipEventElapsedTime(&ms, m.ev[0], m.ev[1]));
        if (report.on) {
            HIP_CHECK(hipEventElapsedTime(&ms_report, report_ev[0], report_ev[1]));
            std::lock_guard<std::mutex> lk(report.mu);
            report.ms += ms_report;
            report.launches++;
        }
        if (match.mode != MTSV_MATCH_OFF) {
            HIP_CHECK(hipEventElapsedTime(&ms_match, match_ev[0], match_ev[1]));
            std::lock_guard<std::mutex> lk(match.mu);
            match.ms += ms_match;
            match.launches++;
        }
    }
    n_hits_total = total;
    total_hits = total;
    segments.push_back(Segment{this, 0, total, 0, n, 0, n_assign});
    stats.n_reads = n;
    stats.n_hits = total;
    last_run = kRunMerged;
    if (device_ms) *device_ms = ms;
    if (getenv("MTSV_TRACE"))
        fprintf(stderr, "[merge] %d sources in %llu stretches, %llu reads, %llu hits: merge kernels %.3f ms, report %.3f ms, flags %.3f ms; %llu bytes to the host, %llu to the device\n",
                n_srcs, (unsigned long long)parts.size(), (unsigned long long)n, (unsigned long long)total, ms, ms_report, ms_match, (unsigned long long)16,
                (unsigned long long)(parts.size() * sizeof(MergePart)));
    if (collapse_on && assign.trace) collapse_trace("merge");
}

void Batch::read_map(std::vector<uint64_t>& map) {
    map.resize(n_reads);
    if (!mapped) {
        for (uint64_t i = 0; i < n_reads; i++) map[i] = i;
        return;
    }
    std::vector<uint32_t> m32(n_reads);
    HIP_CHECK(hipSetDevice(di->device));
    if (n_reads) HIP_CHECK(hipMemcpyAsync(m32.data(), d_read_map.p, n_reads * 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (uint64_t i = 0; i < n_reads; i++) map[i] = m32[i];
}

void Batch::download_reads(std::vector<uint8_t>& codes, std::vector<uint64_t>& read_off) {
    if (!resident) throw std::runtime_error("arg: the workspace holds no resident batch (mtsv_batch_upload, mtsv_batch_take_reads)");
    HIP_CHECK(hipSetDevice(di->device));
    const uint64_t nb = h_read_off[n_reads];
    // (an uploaded batch is normalised into d_codes as run() would do it)
    if (!codes_resident && nb) launch_normalise(stream, d_bases.p, d_codes.p, 0, nb);
    codes.resize(nb);
    if (nb) HIP_CHECK(hipMemcpyAsync(codes.data(), d_codes.p, nb, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    read_off.assign(h_read_off.begin(), h_read_off.begin() + n_reads + 1);
}

// ---------------------------------------------------------------------------------------------
// Pinned result arrays.  The hits of a run travel to page-locked host memory slice by slice while later
// slices still compute, and that array itself is what the caller receives (mtsv_hits_free hands it back
// to this pool), so no copy into fresh malloc memory -- page faults at ~12 GB/s -- sits behind the kernels.
// ---------------------------------------------------------------------------------------------
namespace {
struct PinnedPool {
    std::mutex mu;
    std::vector<std::pair<void*, uint64_t>> free_list;  // (pointer, bytes)
    std::vector<std::pair<void*, uint64_t>> live;
    static constexpr size_t kKeep = 6;  // idle arrays kept for reuse
    void* get(uint64_t bytes, uint64_t* cap) {
        {
            std::lock_guard<std::mutex> lk(mu);
            size_t best = free_list.size();
            for (size_t i = 0; i < free_list.size(); i++)
                if (free_list[i].second >= bytes && (best == free_list.size() || free_list[i].second < free_list[best].second)) best = i;
            if (best != free_list.size()) {
                auto e = free_list[best];
                free_list.erase(free_list.begin() + best);
                live.push_back(e);
                *cap = e.second;
                return e.first;
            }
        }
        void* p = nullptr;
        const uint64_t b = std::max<uint64_t>((bytes + (bytes >> 3) + 4095) & ~4095ull, 1ull << 16);
        HIP_CHECK(hipHostMalloc(&p, b, hipHostMallocPortable));
        std::lock_guard<std::mutex> lk(mu);
        live.emplace_back(p, b);
        *cap = b;
        return p;
    }
    bool put(void* p) {  // false: not one of ours
        std::pair<void*, uint64_t> drop{nullptr, 0};
        {
            std::lock_guard<std::mutex> lk(mu);
            size_t i = 0;
            while (i < live.size() && live[i].first != p) i++;
            if (i == live.size()) return false;
            auto e = live[i];
            live.erase(live.begin() + i);
            free_list.push_back(e);
            if (free_list.size() > kKeep) {  // drop the smallest
                size_t m = 0;
                for (size_t k = 1; k < free_list.size(); k++)
                    if (free_list[k].second < free_list[m].second) m = k;
                drop = free_list[m];
                free_list.erase(free_list.begin() + m);
            }
        }
        if (drop.first) (void)hipHostFree(drop.first);
        return true;
    }
};
PinnedPool& pool() {
    static PinnedPool* p = new PinnedPool;  // never destroyed: arrays may outlive static destruction order
    return *p;
}
}  // namespace

mtsv_hit* pinned_hits_alloc(uint64_t n_hits, uint64_t* cap_hits) {
    uint64_t cap = 0;
    void* p = pool().get(std::max<uint64_t>(n_hits, 1) * sizeof(mtsv_hit), &cap);
    *cap_hits = cap / sizeof(mtsv_hit);
    return (mtsv_hit*)p;
}
bool pinned_hits_release(void* p) { return p && pool().put(p); }

// (a fresh page-locked array costs ~60 us per MB to create and is slow on its first copy: ask for little more than the
//  last batch needed, so that the array that batch returned to the pool fits again)
void PinnedStage::begin(uint64_t expected_first) {
    if (p) return;
    uint64_t units = 0;
    p = (uint8_t*)pinned_hits_alloc(((last_total ? last_total + last_total / 64 : expected_first) * rec + 31) / 32, &units);
    cap = units * 32 / rec;
}

// grown geometrically through the pool (mu of the host run held)
void PinnedStage::reserve(uint64_t need, hipStream_t stream) {
    if (need <= cap) return;
    if (getenv("MTSV_TRACE")) fprintf(stderr, "[run_host] %s array grows %llu -> %llu %s\n", name, (unsigned long long)cap, (unsigned long long)need, unit);
    HIP_CHECK(hipStreamSynchronize(stream));
    uint64_t units = 0;
    auto* q = (uint8_t*)pinned_hits_alloc((std::max<uint64_t>(2 * cap, need) * rec + 31) / 32, &units);
    if (staged) memcpy(q, p, staged * rec);
    pinned_hits_release(p);
    p = q;
    cap = units * 32 / rec;
}

void* PinnedStage::hand_out() {
    void* out = p;
    p = nullptr;
    cap = 0;
    valid = false;
    return out;
}

void PinnedStage::drop() {
    pinned_hits_release(hand_out());
    staged = 0;
}

// The result array is pinned host memory from the pool; the caller owns it until mtsv_hits_free.
void Batch::download(mtsv_hit** hits, uint64_t* n) {
    HIP_CHECK(hipSetDevice(di->device));
    hits_stage.last_total = total_hits;
    if (assign.mode != MTSV_ASSIGN_ONLY && host_hits_dropped)
        throw std::runtime_error("arg: the last run was a host batch in MTSV_ASSIGN_ONLY, which kept none of its hits: run again in the new mode");
    if (assign.mode == MTSV_ASSIGN_ONLY) {  // the hits stay where they are
        uint64_t cap = 0;
        *hits = pinned_hits_alloc(0, &cap);
        *n = 0;
        return;
    }
    if (hits_stage.valid && hits_stage.p) {  // run_host already brought them over
        *hits = (mtsv_hit*)hits_stage.hand_out();
        *n = total_hits;
        return;
    }
    uint64_t cap = 0;
    mtsv_hit* h = pinned_hits_alloc(total_hits, &cap);
    uint64_t at = 0;
    for (auto& sg : segments) {
        if (!sg.count) continue;
        hipError_t e = hipMemcpy(h + at, sg.lane->d_hits.p + sg.offset, sg.count * sizeof(mtsv_hit), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            pinned_hits_release(h);
            throw_hip(e, "hipMemcpy(hits)", __FILE__, __LINE__);
        }
        at += sg.count;
    }
    *hits = h;
    *n = total_hits;
}

void Batch::download_into(mtsv_hit* dst, uint64_t n) {
    HIP_CHECK(hipSetDevice(di->device));
    if (n != total_hits) throw std::runtime_error("internal: download_into of " + std::to_string(n) + " hits, the run produced " + std::to_string(total_hits));
    hits_stage.last_total = total_hits;
    hipStream_t cs = copy_stream2 ? copy_stream2.s : stream.s;
    uint64_t at = 0;
    for (auto& sg : segments) {
        if (!sg.count) continue;
        HIP_CHECK(hipMemcpyAsync(dst + at, sg.lane->d_hits.p + sg.offset, sg.count * sizeof(mtsv_hit), hipMemcpyDeviceToHost, cs));
        at += sg.count;
    }
    HIP_CHECK(hipStreamSynchronize(cs));
}

}  // namespace mtsv
