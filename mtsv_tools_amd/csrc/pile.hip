// pile.hip -- mtsv_pileup (include/mtsv_amd.h): what the reads that align over a reference position show there, by the kernels
// of k_pile.hip.  add_run places the hits first (place.hip, without its copies to the host), then plans the references on the
// host and allocates a new segment, then counts the hits that count -- and only then piles.  Every refusal lies before the pile
// kernel, the only writer of counters: a refused call leaves the accumulator byte for byte as it was, a segment that was
// allocated for it is dropped before it joins the table.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "batch.hpp"
#include "pile.hpp"
#include "place.hpp"

namespace mtsv {

namespace {

// DevBuf says "device: no memory for ...": of a segment that is MTSV_E_NOMEM
template <class F>
void as_nomem(F&& alloc) {
    try {
        alloc();
    } catch (const std::runtime_error& e) {
        const std::string m = e.what();
        if (m.rfind("device: no memory", 0) == 0) throw std::runtime_error("nomem:" + m.substr(7));
        throw;
    }
}

}  // namespace

Pileup::Pileup(int device_, const uint32_t* taxa, uint64_t n_taxa) : device(device_) {
    require_device(device);
    refs.set_taxa(taxa, n_taxa);
    tile = tile_from_env("MTSV_PILE_TILE", kPileTile, 64, kPileTileMax);
    if (const char* e = getenv("MTSV_CONS_WRITE")) cons_staged = std::string(e) == "staged" ? true : std::string(e) == "plain" ? false : cons_staged;
    trace = getenv("MTSV_TRACE") != nullptr;
    timing = getenv("MTSV_PILE_TIMING") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    stream.create(hipStreamNonBlocking);
    ev.create();
}

Pileup::~Pileup() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    if (stream.s) (void)hipStreamSynchronize(stream);
}

void Pileup::reset() {
    HIP_CHECK(hipSetDevice(device));
    for (auto& sg : segs) HIP_CHECK(hipMemsetAsync(sg->cnt.p, 0, (uint64_t)sg->n_slots * 8 * sizeof(uint32_t), stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    hits_piled = hits_skipped = 0;
}

void Pileup::info(mtsv_pileup_info_t* out) const {
    uint64_t bytes = 0;
    for (const auto& sg : segs) bytes += sg->bytes();
    *out = mtsv_pileup_info_t{refs.refs.size(), refs.n_slots(), segs.size(), bytes, hits_piled, hits_skipped};
}

// the new references of a plan: zeroed counters, the ref codes copied from the workspace's resident text.  Not in the table yet.
std::unique_ptr<Pileup::Segment> Pileup::make_segment(Batch& b, const PileRefs::Plan& plan) {
    auto sg = std::make_unique<Segment>();
    const uint64_t n_refs = plan.fresh.size();
    sg->n_slots = (uint32_t)plan.n_slots;
    sg->n_refs = (uint32_t)n_refs;
    as_nomem([&] {
        sg->cnt.alloc(plan.n_slots * 8, "the pileup segment's counters");
        sg->ref.alloc(plan.n_slots, "the pileup segment's reference codes");
        sg->ref_off.alloc(n_refs + 1, "the pileup segment's first slots");
        sg->ref_key.alloc(n_refs, "the pileup segment's keys");
    });
    std::vector<uint32_t> off(n_refs + 1), start(n_refs);
    std::vector<uint64_t> key(n_refs);
    const std::vector<Bin>& bins = b.ix->host.bins;
    for (uint64_t k = 0; k < n_refs; k++) {
        off[k] = plan.fresh[k].off;
        key[k] = plan.fresh[k].key;
        start[k] = (uint32_t)bins[plan.fresh_bin[k]].start;
    }
    off[n_refs] = sg->n_slots;
    hipStream_t s = b.stream;
    DevBuf<uint32_t> d_start;
    d_start.alloc(n_refs, "the new references' text positions");
    HIP_CHECK(hipMemcpyAsync(sg->ref_off.p, off.data(), (n_refs + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(sg->ref_key.p, key.data(), n_refs * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_start.p, start.data(), n_refs * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(sg->cnt.p, 0, plan.n_slots * 8 * sizeof(uint32_t), s));
    launch_pile_ref(s, b.di->d_text, sg->ref_off.p, d_start.p, sg->n_refs, sg->n_slots, sg->ref.p);
    HIP_CHECK(hipStreamSynchronize(s));  // (the host arrays and d_start go with this frame)
    HIP_CHECK(hipGetLastError());
    return sg;
}

void Pileup::add_run(Batch& b, const mtsv_hit* hits, uint64_t n_hits, uint32_t edit_slack, uint64_t* n_piled, uint64_t* n_skipped, float* device_ms) {
    if (device_ms) *device_ms = 0;
    if (n_piled) *n_piled = 0;
    if (n_skipped) *n_skipped = 0;
    const double t0 = timing ? now_ms() : 0;
    if (b.parent) throw std::runtime_error("internal: a pileup of a lane");
    if (b.di->device != device)
        throw std::runtime_error("arg: the workspace is on device " + std::to_string(b.di->device) + ", the pileup on device " + std::to_string(device));
    // ---- place: everything mtsv_batch_place_hits refuses is refused here, nothing of the accumulator has been touched ----
    if (!b.placer) b.placer = std::make_shared<Placer>(b.di->device);
    Placer& pl = *b.placer;
    Placer::Placed placed;
    pl.place_on_device(b, hits, n_hits, placed);
    if (!placed.n) return;  // nothing is launched, no reference is learnt
    // ---- register: the index's selected bins, the new ones as a segment that is not in the table yet ----
    const std::vector<Bin>& bins = b.ix->host.bins;
    std::vector<uint64_t> key(bins.size()), len(bins.size());
    for (size_t k = 0; k < bins.size(); k++) {
        key[k] = (uint64_t)bins[k].tax_id << 32 | bins[k].gi;
        len[k] = bins[k].end >= bins[k].start ? bins[k].end - bins[k].start : 0;
    }
    const PileRefs::Plan plan = refs.plan(key.data(), len.data(), bins.size(), (uint32_t)segs.size());
    hipStream_t s = b.stream;
    std::unique_ptr<Segment> fresh;
    if (!plan.fresh.empty()) fresh = make_segment(b, plan);
    h_bin_cnt.assign(bins.size(), nullptr);
    for (size_t k = 0; k < bins.size(); k++) {
        if (plan.bin_ref[k] == PileRefs::Plan::kUnselected) continue;
        const PileRefs::Ref& r = PileRefs::of(plan, refs.refs, plan.bin_ref[k]);
        Segment& sg = r.seg < segs.size() ? *segs[r.seg] : *fresh;
        h_bin_cnt[k] = sg.cnt.p + (uint64_t)r.off * 8;
    }
    const uint32_t N = (uint32_t)placed.n, n_bins = (uint32_t)bins.size(), n_reads = (uint32_t)b.n_reads;
    d_bin_cnt.room(s, bins.size(), "the bins' counters");
    d_best.room(s, b.n_reads, "the reads' smallest edits");
    d_ctr.room(s, kPileCounters, "the pileup's counters", 16);
    HIP_CHECK(hipMemcpyAsync(d_bin_cnt.p, h_bin_cnt.data(), bins.size() * sizeof(uint32_t*), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(d_best.p, 0xff, b.n_reads * sizeof(uint32_t), s));
    HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, kPileCounters * sizeof(uint64_t), s));
    // ---- which hits count: scratch and two counters ----
    HIP_CHECK(hipEventRecord(ev[0], s));
    launch_pile_best(s, pl.d_in.p, N, pl.d_hit_read.p, n_reads, d_best.p);
    launch_pile_count(s, pl.d_in.p, N, pl.d_hit_bin.p, pl.d_hit_read.p, n_bins, n_reads, d_best.p, edit_slack, d_bin_cnt.p, d_ctr.p);
    HIP_CHECK(hipEventRecord(ev[1], s));
    uint64_t ctr[kPileCounters] = {};
    HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    // ---- the last refusal point: the counters are 32 bits wide ----
    const uint64_t counted = ctr[kPileCtrCounted], skipped = ctr[kPileCtrSkipped];
    if (counted + skipped > placed.n) throw std::runtime_error("internal: " + std::to_string(placed.n) + " hits, " + std::to_string(counted) + " counted and " +
                                                               std::to_string(skipped) + " skipped");
    if (hits_piled + counted >= (1ull << 32))
        throw std::runtime_error("limit: " + std::to_string(hits_piled) + " hits are piled and this call brings " + std::to_string(counted) +
                                 ": 2^32 or more, and a counter holds 32 bits");
    // ---- pile: nothing is refused from here on ----
    if (fresh) {
        segs.push_back(std::move(fresh));
        refs.commit(plan);
    }
    HIP_CHECK(hipEventRecord(ev[2], s));
    launch_pile(s, pl.d_in.p, N, pl.d_hit_bin.p, pl.d_hit_read.p, b.di->d_bins, n_bins, n_reads, d_best.p, edit_slack, d_bin_cnt.p, b.d_codes.p, b.d_read_off.p,
                pl.d_out.p, pl.d_ops.p, placed.total_ops, d_ctr.p);
    HIP_CHECK(hipEventRecord(ev[3], s));
    HIP_CHECK(hipMemcpyAsync(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    HIP_CHECK(hipGetLastError());
    hits_piled += counted;
    hits_skipped += skipped;
    if (ctr[kPileCtrBroken])
        throw std::runtime_error("internal: " + std::to_string(ctr[kPileCtrBroken]) + " of " + std::to_string(counted) + " edit scripts left their reference's slots");
    float ms_best = 0, ms_pile = 0;
    HIP_CHECK(hipEventElapsedTime(&ms_best, ev[0], ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms_pile, ev[2], ev[3]));
    const float ms_all = placed.ms_map + placed.ms_place + ms_best + ms_pile;
    if (device_ms) *device_ms = ms_all;
    if (n_piled) *n_piled = counted;
    if (n_skipped) *n_skipped = skipped;
    if (trace)
        fprintf(stderr, "[pile] %llu hits (%s), %llu piled at slack %u, %llu skipped, %zu new references, %zu segments: %.3f ms\n", (unsigned long long)placed.n,
                placed.own ? "the last run's" : "given", (unsigned long long)counted, edit_slack, (unsigned long long)skipped, plan.fresh.size(), segs.size(), ms_all);
    // MTSV_PILE_TIMING=1: where a call spends its time (tools/pile_ab.py reads this line)
    if (timing)
        fprintf(stderr, "[pile timing] add_run hits %llu piled %llu skipped %llu op_slots %llu new_refs %zu; place_scan %.3f ms, place %.3f ms, best %.3f ms, "
                        "pile %.3f ms, call %.3f ms\n",
                (unsigned long long)placed.n, (unsigned long long)counted, (unsigned long long)skipped, (unsigned long long)placed.total_ops, plan.fresh.size(),
                placed.ms_map, placed.ms_place, ms_best, ms_pile, now_ms() - t0);
}

void Pileup::integrate(Segment& sg) {
    const uint32_t tiles = pile_tiles(sg.n_slots, tile);
    d_tile_sum.room(stream, tiles, "the tiles' sums");
    d_tile_pre.room(stream, (uint64_t)tiles + 1, "the tiles' prefixes");
    d_sums.room(stream, (uint64_t)scan_tiles(tiles) + 2, "the scan's sums");
    launch_pile_tile_sums(stream, sg.cnt.p, sg.n_slots, tile, d_tile_sum.p);
    launch_scan(stream, d_tile_sum.p, tiles, d_sums.p + 1, d_sums.p, d_tile_pre.p);
}

void Pileup::download(uint32_t tax_id, uint32_t gi, std::vector<uint32_t>& counts, std::vector<uint8_t>& ref) {
    const PileRefs::Ref* r = refs.find((uint64_t)tax_id << 32 | gi);
    if (!r) throw std::runtime_error("arg: the pileup holds no reference (tax_id " + std::to_string(tax_id) + ", gi " + std::to_string(gi) + ")");
    HIP_CHECK(hipSetDevice(device));
    Segment& sg = *segs[r->seg];
    const uint64_t n = (uint64_t)r->len + 1;
    counts.resize(n * 8);
    ref.resize(n);
    d_dump.room(stream, n * 8, "the downloaded counters");
    integrate(sg);
    launch_pile_dump(stream, sg.cnt.p, sg.n_slots, tile, d_tile_pre.p, r->off, (uint32_t)(r->off + n), d_dump.p);
    HIP_CHECK(hipMemcpyAsync(counts.data(), d_dump.p, n * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(ref.data(), sg.ref.p + r->off, n, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
}

void Pileup::sites(uint32_t min_depth, uint32_t min_alt, uint32_t min_alt_ppm, std::vector<mtsv_pile_site>& rows, float* device_ms) {
    static_assert(sizeof(mtsv_pile_site) == 48, "k_pile_sites writes a row as twelve words");
    if (device_ms) *device_ms = 0;
    rows.clear();
    const double t0 = timing ? now_ms() : 0;
    float ms_all = 0;
    HIP_CHECK(hipSetDevice(device));
    for (auto& sgp : segs) {
        Segment& sg = *sgp;
        const uint32_t tiles = pile_tiles(sg.n_slots, tile);
        d_tile_cnt.room(stream, tiles, "the tiles' sites");
        d_tile_off.room(stream, (uint64_t)tiles + 1, "the tiles' first rows");
        HIP_CHECK(hipEventRecord(ev[4], stream));
        integrate(sg);
        launch_pile_sites_count(stream, sg.cnt.p, sg.n_slots, tile, d_tile_pre.p, min_depth, min_alt, min_alt_ppm, d_tile_cnt.p);
        launch_scan(stream, d_tile_cnt.p, tiles, d_sums.p + 1, d_sums.p, d_tile_off.p);
        uint64_t n_rows = 0;
        HIP_CHECK(hipMemcpyAsync(&n_rows, d_sums.p, sizeof n_rows, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        if (n_rows > sg.n_slots) throw std::runtime_error("internal: " + std::to_string(n_rows) + " sites in a segment of " + std::to_string(sg.n_slots) + " slots");
        d_rows.room(stream, n_rows * sizeof(mtsv_pile_site), "the sites' rows");
        launch_pile_sites_rows(stream, sg.cnt.p, sg.n_slots, tile, d_tile_pre.p, min_depth, min_alt, min_alt_ppm, d_tile_off.p, sg.ref_off.p, sg.ref_key.p,
                               sg.n_refs, sg.ref.p, d_rows.p, n_rows);
        HIP_CHECK(hipEventRecord(ev[5], stream));
        const size_t at = rows.size();
        rows.resize(at + n_rows);
        if (n_rows) HIP_CHECK(hipMemcpyAsync(rows.data() + at, d_rows.p, n_rows * sizeof(mtsv_pile_site), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ev[4], ev[5]));
        ms_all += ms;
    }
    // (a segment's rows ascend: its references lie in key order; the segments' ranges of keys interleave)
    auto before = [](const mtsv_pile_site& a, const mtsv_pile_site& b) {
        return a.tax_id != b.tax_id ? a.tax_id < b.tax_id : a.gi != b.gi ? a.gi < b.gi : a.pos < b.pos;
    };
    if (segs.size() > 1 && !std::is_sorted(rows.begin(), rows.end(), before)) std::sort(rows.begin(), rows.end(), before);
    if (device_ms) *device_ms = ms_all;
    if (timing)
        fprintf(stderr, "[pile timing] sites segments %zu slots %llu tile %u rows %zu; sites %.3f ms, call %.3f ms\n", segs.size(),
                (unsigned long long)refs.n_slots(), tile, rows.size(), ms_all, now_ms() - t0);
}

}  // namespace mtsv
