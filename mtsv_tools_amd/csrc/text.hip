// text.hip -- the results file's lines written on the device (mtsv_fold_format_text, mtsv_batch_format_text,
// include/mtsv_amd.h): the records are in HBM already, the read IDs go up, k_text.hip measures, scans and writes, and
// what crosses to the host is the text.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "batch.hpp"
#include "fold.hpp"
#include "text.hpp"

namespace mtsv {

TextFormatter::TextFormatter(int device_) : device(device_) {
    tile = tile_from_env("MTSV_TEXT_TILE", kTextTile, 2, kTextTileMax);
    trace = getenv("MTSV_TRACE") != nullptr;
    timing = getenv("MTSV_TEXT_TIMING") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    ev.create();
}

TextFormatter::~TextFormatter() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    if (stream) (void)hipStreamSynchronize(stream);
    if (stream) (void)hipStreamDestroy(stream);
}

void TextFormatter::format(int grain, const std::vector<Stretch>& src, const char* ids, const uint64_t* id_off, uint64_t n_reads, char** text,
                           uint64_t* len, float* device_ms) {
    const uint64_t rec = grain == MTSV_GRAIN_TAXID ? sizeof(mtsv_assignment) : sizeof(mtsv_assignment_gi);
    uint64_t n = 0, n_src = 0;
    for (const auto& s : src) n += s.n, n_src += s.n != 0;
    if (n >= (1ull << 32)) throw std::runtime_error("limit: the text of " + std::to_string(n) + " records, 2^32 or more");
    const uint32_t tiles = text_tiles(n, tile);
    if (tiles > 0x7fffffffu) throw std::runtime_error("limit: " + std::to_string(tiles) + " tiles of " + std::to_string(tile) + " records");
    HIP_CHECK(hipSetDevice(device));
    if (device_ms) *device_ms = 0;
    uint64_t pool_cap = 0;
    if (!n) {
        char* out = (char*)pinned_hits_alloc(1, &pool_cap);
        out[0] = 0;
        *text = out;
        *len = 0;
        return;
    }
    // ---- the IDs go up; the records come to lie next to each other ----
    const double t0 = timing ? now_ms() : 0;
    const uint64_t ids_bytes = n_reads ? id_off[n_reads] : 0;
    d_ids.room(stream, ids_bytes + 8, "the read IDs");
    d_id_off.room(stream, n_reads + 1, "the read IDs' offsets");
    if (ids_bytes) HIP_CHECK(hipMemcpyAsync(d_ids.p, ids, ids_bytes, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_id_off.p, id_off, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    if (timing) HIP_CHECK(hipStreamSynchronize(stream));
    const double t1 = timing ? now_ms() : 0;
    const uint8_t* d_rec = nullptr;
    if (n_src == 1) {
        for (const auto& s : src)
            if (s.n) d_rec = s.rec;
    } else {
        d_gather.room(stream, n * rec, "the gathered records");
        uint64_t at = 0;
        for (const auto& s : src) {
            if (!s.n) continue;
            HIP_CHECK(hipMemcpyAsync(d_gather.p + at * rec, s.rec, s.n * rec, hipMemcpyDeviceToDevice, stream));
            at += s.n;
        }
        d_rec = d_gather.p;
    }
    d_rec_len.room(stream, n, "the records' lengths");
    d_tile_cnt.room(stream, tiles, "the tiles' lengths");
    d_tile_off.room(stream, (uint64_t)tiles + 1, "the tiles' offsets");
    d_sums.room(stream, (uint64_t)text_scan_blocks(tiles) + 3, "the scan's sums");
    uint64_t* d_total = d_sums.p + text_scan_blocks(tiles);
    // ---- measure and scan; the host needs the length before the text has a place ----
    uint64_t res[3] = {0, 0, 0};  // the bytes of the text, the reads beyond n_reads, the bad ID slots
    HIP_CHECK(hipMemsetAsync(d_total, 0, sizeof res, stream));
    HIP_CHECK(hipEventRecord(ev[0], stream));
    launch_text_measure(stream, grain, d_rec, (uint32_t)n, d_ids.p, d_id_off.p, n_reads, ids_bytes, tile, d_rec_len.p, d_tile_cnt.p, d_total + 1);
    launch_text_scan(stream, d_tile_cnt.p, tiles, d_sums.p, d_total, d_tile_off.p);
    HIP_CHECK(hipEventRecord(ev[1], stream));
    HIP_CHECK(hipMemcpyAsync(res, d_total, sizeof res, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (res[1])
        throw std::runtime_error("arg: " + std::to_string(res[1]) + " reads of the records are numbered at or above the " + std::to_string(n_reads) +
                                 " reads of the ID table");
    if (res[2])
        throw std::runtime_error("arg: " + std::to_string(res[2]) + " ID slots do not lie inside the ID bytes (id_off must ascend) or are longer than " +
                                 std::to_string(kTextIdMax) + " bytes");
    const uint64_t total = res[0];
    d_out.room(stream, total + 16, "the text");
    char* out = (char*)pinned_hits_alloc((total + 1 + 31) / 32, &pool_cap);  // (the pool counts in 32-byte hits)
    // ---- write, and the text comes down ----
    float ms = 0, ms2 = 0;
    double t2 = 0, t3 = 0;
    try {
        HIP_CHECK(hipEventRecord(ev[2], stream));
        launch_text_write(stream, grain, d_rec, (uint32_t)n, d_ids.p, d_id_off.p, tile, d_rec_len.p, d_tile_off.p, d_out.p);
        HIP_CHECK(hipEventRecord(ev[3], stream));
        if (timing) {
            HIP_CHECK(hipStreamSynchronize(stream));
            t2 = now_ms();
        }
        if (total) HIP_CHECK(hipMemcpyAsync(out, d_out.p, total, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        if (timing) t3 = now_ms();
        HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        HIP_CHECK(hipEventElapsedTime(&ms2, ev[2], ev[3]));
    } catch (...) {
        pinned_hits_release(out);
        throw;
    }
    out[total] = 0;
    ms += ms2;
    if (trace)
        fprintf(stderr, "[text] %llu records -> %llu bytes in %u tiles of %u (windows of %u bytes): %.3f ms\n", (unsigned long long)n, (unsigned long long)total,
                tiles, tile, text_window_bytes(tile), ms);
    // MTSV_TEXT_TIMING=1: where a call spends its time (tools/text_ab.py reads this line)
    if (timing)
        fprintf(stderr, "[text timing] records %llu id_bytes %llu text_bytes %llu; id_upload %.3f ms, kernels %.3f ms, text_copy %.3f ms\n", (unsigned long long)n,
                (unsigned long long)(ids_bytes + (n_reads + 1) * 8), (unsigned long long)total, t1 - t0, ms, t3 - t2);
    *text = out;
    *len = total;
    if (device_ms) *device_ms = ms;
}

void Fold::format_text(const char* ids, const uint64_t* id_off, uint64_t n_reads_, char** text_out, uint64_t* len, float* device_ms) {
    if (n_reads_ != n_reads)
        throw std::runtime_error("arg: the ID table has " + std::to_string(n_reads_) + " reads, the fold was reset for " + std::to_string(n_reads));
    HIP_CHECK(hipSetDevice(device));
    if (!text) {
        text.reset(new TextFormatter(device));
        text->tile = text_tile;  // (read when the fold was created)
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    text->format(grain, {TextFormatter::Stretch{d_rec[cur].p, n}}, ids, id_off, n_reads, text_out, len, device_ms);
}

void Batch::format_text(const char* ids, const uint64_t* id_off, uint64_t n_reads_, char** text_out, uint64_t* len, float* device_ms) {
    if (parent) throw std::runtime_error("internal: text of a lane");
    if (assign.mode == MTSV_ASSIGN_OFF) throw std::runtime_error("arg: the assignments of the workspace are not switched on (mtsv_batch_set_assignments)");
    if (last_run == kRunHostOneSegment || last_run == kRunHostSegments)
        throw std::runtime_error("arg: the workspace's last run was a host batch, whose records left for the host range by range (the text is written from a run on a "
                                 "resident batch: mtsv_batch_upload / _take_reads / _copy_reads + mtsv_batch_run, or mtsv_batch_merge_runs)");
    if (last_run != kRunResident && last_run != kRunMerged)
        throw std::runtime_error("arg: the workspace has no completed run on a resident batch whose assignments are still in HBM");
    HIP_CHECK(hipSetDevice(di->device));
    if (!text) text = std::make_shared<TextFormatter>(di->device);
    const uint64_t rec = assign.rec_bytes();
    std::vector<TextFormatter::Stretch> src;
    // (the run has returned: nothing of the workspace is in flight)
    for (const auto& sg : segments)
        if (sg.a_count) src.push_back(TextFormatter::Stretch{sg.lane->d_assign.p + sg.a_offset * rec, sg.a_count});
    text->format(assign.grain, src, ids, id_off, n_reads_, text_out, len, device_ms);
}

}  // namespace mtsv
