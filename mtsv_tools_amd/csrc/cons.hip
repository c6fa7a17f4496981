// cons.hip -- mtsv_pileup_consensus and mtsv_pileup_add_counts (include/mtsv_amd.h, "consensus"): the host side of k_cons.hip.
// Per segment, on the accumulator's stream: integrate (pile.hip), the call pass, and -- when the text is asked for -- the scan of
// the tiles' characters, the layout, the headers and the write pass; the cells, the layout and the text come to the host per
// segment.  The accumulator's references ascend by key over all segments (PileRefs::refs) and a segment's references ascend by
// key too, so the k-th reference of a segment met on the way through the table is that segment's reference k: the rows and the
// text pieces are interleaved by one walk over the table.  Nothing of a segment is written: every refusal leaves the accumulator
// as it was.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "cons_rows.hpp"
#include "pile.hpp"

namespace mtsv {

namespace {

template <class F>
void cons_as_nomem(F&& alloc) {
    try {
        alloc();
    } catch (const std::runtime_error& e) {
        const std::string m = e.what();
        if (m.rfind("device: no memory", 0) == 0) throw std::runtime_error("nomem:" + m.substr(7));
        throw;
    }
}

}  // namespace

void Pileup::consensus(uint32_t min_depth, uint32_t min_frac_ppm, uint32_t min_breadth_ppm, uint32_t fill, uint32_t line_width, std::vector<char>* fasta,
                       std::vector<mtsv_cons_ref>& rows, float* device_ms) {
    if (device_ms) *device_ms = 0;
    rows.clear();
    if (fasta) fasta->clear();
    if (fill > 1) throw std::runtime_error("arg: a consensus fill of " + std::to_string(fill) + " (0: N, 1: the reference base in lower case)");
    if (min_frac_ppm > 1000000) throw std::runtime_error("arg: a consensus min_frac_ppm of " + std::to_string(min_frac_ppm) + ", above 1000000");
    if (segs.empty()) return;
    const double t0 = timing ? now_ms() : 0;
    const uint32_t md = std::max(min_depth, 1u);
    float ms_call = 0, ms_layout = 0, ms_write = 0;
    HIP_CHECK(hipSetDevice(device));
    std::vector<std::vector<uint32_t>> h_cells(segs.size()), h_lay(segs.size());
    std::vector<std::vector<char>> h_text(segs.size());
    for (size_t g = 0; g < segs.size(); g++) {
        Segment& sg = *segs[g];
        const uint32_t tiles = pile_tiles(sg.n_slots, tile);
        cons_as_nomem([&] {
            d_cells.room(stream, (uint64_t)sg.n_refs * kConsCell, "the consensus calls' cells");
            if (fasta) {
                d_call.room(stream, sg.n_slots, "the consensus calls");
                d_ref_pre.room(stream, sg.n_refs, "the consensus calls' prefixes");
                d_lay.room(stream, (uint64_t)sg.n_refs * kConsLay, "the consensus calls' layout");
            }
        });
        d_tile_cnt.room(stream, tiles, "the tiles' sites");
        d_tile_off.room(stream, (uint64_t)tiles + 1, "the tiles' first rows");
        HIP_CHECK(hipEventRecord(ev[6], stream));
        integrate(sg);
        HIP_CHECK(hipMemsetAsync(d_cells.p, 0, (uint64_t)sg.n_refs * kConsCell * sizeof(uint32_t), stream));
        launch_cons_call(stream, sg.cnt.p, sg.n_slots, tile, d_tile_pre.p, sg.ref_off.p, sg.n_refs, sg.ref.p, md, min_frac_ppm, fill, fasta ? d_call.p : nullptr,
                         d_tile_cnt.p, d_ref_pre.p, d_cells.p);
        HIP_CHECK(hipEventRecord(ev[7], stream));
        h_cells[g].resize((uint64_t)sg.n_refs * kConsCell);
        HIP_CHECK(hipMemcpyAsync(h_cells[g].data(), d_cells.p, h_cells[g].size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        uint64_t total[2] = {0, 0};
        if (fasta) {
            launch_scan(stream, d_tile_cnt.p, tiles, d_sums.p + 1, d_sums.p, d_tile_off.p);
            // (d_sums: integrate gave it scan_tiles(tiles) + 2 entries; the layout's two totals go where the scan's total was)
            launch_cons_layout(stream, d_cells.p, sg.ref_off.p, sg.ref_key.p, sg.n_refs, d_ref_pre.p, d_tile_off.p, tile, min_breadth_ppm, line_width, d_lay.p,
                               d_sums.p);
            HIP_CHECK(hipEventRecord(ev[8], stream));
            HIP_CHECK(hipMemcpyAsync(total, d_sums.p, sizeof total, hipMemcpyDeviceToHost, stream));
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, ev[6], ev[7]));
        ms_call += ms;
        if (!fasta) continue;
        HIP_CHECK(hipEventElapsedTime(&ms, ev[7], ev[8]));
        ms_layout += ms;
        if (total[0] >= (1ull << 32))
            throw std::runtime_error("limit: the consensus text of segment " + std::to_string(g) + " takes " + std::to_string(total[0]) +
                                     " bytes, 2^32 or more: select fewer TaxIDs or raise the breadth threshold");
        cons_as_nomem([&] { d_text.room(stream, total[0], "the consensus text"); });
        HIP_CHECK(hipEventRecord(ev[8], stream));
        launch_cons_write(stream, d_call.p, sg.n_slots, tile, d_tile_off.p, sg.ref_off.p, sg.ref_key.p, sg.n_refs, d_lay.p, line_width, d_text.p, total[0], cons_staged);
        HIP_CHECK(hipEventRecord(ev[9], stream));
        h_lay[g].resize((uint64_t)sg.n_refs * kConsLay);
        h_text[g].resize(total[0]);
        HIP_CHECK(hipMemcpyAsync(h_lay[g].data(), d_lay.p, h_lay[g].size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        if (total[0]) HIP_CHECK(hipMemcpyAsync(h_text[g].data(), d_text.p, total[0], hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&ms, ev[8], ev[9]));
        ms_write += ms;
    }
    // ---- the rows, and the text pieces of several segments, in the table's order ----
    std::vector<uint32_t> next(segs.size(), 0);
    const bool pieces = fasta && segs.size() > 1;
    for (const PileRefs::Ref& r : refs.refs) {
        const uint32_t k = next[r.seg]++;
        const uint32_t* cell = h_cells[r.seg].data() + (uint64_t)k * kConsCell;
        const mtsv_cons_ref row = cons_row((uint32_t)(r.key >> 32), (uint32_t)r.key, r.len, cell);
        if (!cons_emitted(row, min_breadth_ppm)) continue;
        rows.push_back(row);
        if (!fasta) continue;
        const uint32_t* q = h_lay[r.seg].data() + (uint64_t)k * kConsLay;
        const uint64_t at = (uint64_t)q[0] | (uint64_t)q[1] << 32, bytes = (uint64_t)q[6] | (uint64_t)q[7] << 32;
        if (!q[5] || at + bytes > h_text[r.seg].size()) throw std::runtime_error("internal: the consensus layout of (tax_id " + std::to_string(row.tax_id) + ", gi " +
                                                                                  std::to_string(row.gi) + ") disagrees with its row");
        if (pieces) fasta->insert(fasta->end(), h_text[r.seg].begin() + at, h_text[r.seg].begin() + at + bytes);
    }
    if (fasta && !pieces) fasta->swap(h_text[0]);
    const float ms_all = ms_call + ms_layout + ms_write;
    if (device_ms) *device_ms = ms_all;
    if (timing)
        fprintf(stderr, "[pile timing] consensus segments %zu slots %llu tile %u rows %zu bytes %zu write %s; call %.3f ms, layout %.3f ms, write %.3f ms, call_all %.3f ms\n",
                segs.size(), (unsigned long long)refs.n_slots(), tile, rows.size(), fasta ? fasta->size() : (size_t)0, cons_staged ? "staged" : "plain", ms_call, ms_layout, ms_write,
                now_ms() - t0);
}

void Pileup::add_counts(uint32_t tax_id, uint32_t gi, uint32_t first_slot, uint64_t n_slots, const uint32_t* counts, uint64_t n_hits) {
    const PileRefs::Ref* r = refs.find((uint64_t)tax_id << 32 | gi);
    if (!r) throw std::runtime_error("arg: the pileup holds no reference (tax_id " + std::to_string(tax_id) + ", gi " + std::to_string(gi) + ")");
    const uint64_t slots = (uint64_t)r->len + 1;
    if ((uint64_t)first_slot + n_slots > slots)
        throw std::runtime_error("arg: slots " + std::to_string(first_slot) + " .. " + std::to_string((uint64_t)first_slot + n_slots - 1) + " of a reference of " +
                                 std::to_string(slots) + " slots");
    for (uint64_t k = 0; k < n_slots; k++)
        for (int c = 0; c < 8; c++) {
            const uint32_t v = counts[k * 8 + c];
            if (v > n_hits)
                throw std::runtime_error("arg: a count of " + std::to_string(v) + " at slot " + std::to_string(first_slot + k) + " with " + std::to_string(n_hits) +
                                         " hits: no counter may take more than the hits that are added");
            if (v && c < 7 && first_slot + k == r->len)
                throw std::runtime_error("arg: slot L (" + std::to_string(r->len) + ") takes insertions only, and channel " + std::to_string(c) + " is given " +
                                         std::to_string(v));
        }
    if (hits_piled + n_hits >= (1ull << 32))
        throw std::runtime_error("limit: " + std::to_string(hits_piled) + " hits are piled and this call brings " + std::to_string(n_hits) +
                                 ": 2^32 or more, and a counter holds 32 bits");
    HIP_CHECK(hipSetDevice(device));
    if (n_slots) {
        Segment& sg = *segs[r->seg];
        cons_as_nomem([&] { d_add.room(stream, n_slots * 8, "the added counts"); });
        HIP_CHECK(hipMemcpyAsync(d_add.p, counts, n_slots * 8 * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        launch_cons_add(stream, sg.cnt.p + (uint64_t)r->off * 8, (uint32_t)slots, first_slot, n_slots, d_add.p);
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
    }
    hits_piled += n_hits;
}

}  // namespace mtsv
