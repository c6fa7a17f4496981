// dedup.hip -- identical reads binned once (mtsv_dupmap, include/mtsv_amd.h; kernels in k_dedup.hip).
//
// The result of binning is a function of a read's codes and the parameters, so a batch that holds a sequence many times --
// PCR and optical duplicates, rRNA, amplicons -- needs the seed, coalesce and verify kernels once per distinct sequence.
// take_unique finds the groups of identical reads of a resident batch and packs the first read of every group into another
// workspace, with the kernels mtsv_batch_take_reads packs the unmatched reads with; the run and the fold see the
// representatives; expand fans the representatives' records out to every read, so that the fold everything is derived from is
// the one the whole batch would have given.  The reads, their codes and the records stay in HBM: the host reads five counters
// and the survivors' offsets in a take, two counters in an expansion.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "dedup.hpp"

namespace mtsv {

DupMap::DupMap(int device_) : device(device_) {
    require_device(device);
    if (const char* e = getenv("MTSV_DEDUP_HASH_BITS")) hash_bits = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), 64);  // (tests: long chains, equal tags)
    fan_tile = tile_from_env("MTSV_FAN_TILE", kFanTile, 64, kFanTileMax);
    trace = getenv("MTSV_TRACE") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    ev.create();
    fan.ev.create();
}

DupMap::~DupMap() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
}

void DupMap::take_unique(Batch& dst, Batch& src, uint64_t* n_unique_out, uint64_t* bases_kept, float* device_ms) {
    if (dst.parent || src.parent) throw std::runtime_error("internal: take_unique on a lane");
    if (&src == &dst) throw std::runtime_error("arg: take_unique from a workspace into itself");
    if (src.di->device != dst.di->device) throw std::runtime_error("arg: take_unique between workspaces of different devices");
    if (device != dst.di->device) throw std::runtime_error("arg: the map is on device " + std::to_string(device) + ", the workspaces on device " + std::to_string(dst.di->device));
    const bool host_batch = !src.resident && src.last_run == Batch::kRunHostOneSegment;
    if (!src.resident && !host_batch)
        throw std::runtime_error("arg: the source workspace holds no resident batch (mtsv_batch_upload, mtsv_batch_take_reads, mtsv_batch_copy_reads, or a host batch of one input segment)");
    const uint64_t n_src = src.n_reads;
    if (n_src > (1ull << 30)) throw std::runtime_error("limit: more than 2^30 reads in one take_unique (the table's slots are numbered in 32 bits)");
    const uint32_t* ho = host_batch ? src.h_off_all.p : src.h_read_off.data();
    const uint64_t nb_src = n_src ? ho[n_src] : 0;
    const bool codes = host_batch || src.codes_resident;
    const uint8_t* s_codes = host_batch ? src.arena[0].d_bases.p : src.d_codes.p;
    const uint32_t* s_off = host_batch ? src.arena[0].d_off.p : src.d_read_off.p;
    const uint32_t* s_map = !host_batch && src.mapped ? src.d_read_map.p : nullptr;
    HIP_CHECK(hipSetDevice(device));
    hipStream_t stream = dst.stream;
    // ---- room: the map's (a refusal from here on leaves both the map and dst as they were) ----
    uint64_t slots = 2;
    while (slots < 2 * n_src) slots *= 2;
    if (n_src > d_read[0].cap || !d_read[0].p) {
        // (four new arrays; the map's entries move to the first of each pair, and the old arrays leave with `fresh`)
        DevBuf<uint32_t> fresh[4];
        for (auto& b : fresh) b.room(stream, n_src, "the map");
        if (valid && n) {
            HIP_CHECK(hipMemcpyAsync(fresh[0].p, d_read[cur].p, n * 4, hipMemcpyDeviceToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(fresh[2].p, d_rep[cur].p, n * 4, hipMemcpyDeviceToDevice, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        }
        for (int k = 0; k < 2; k++) {
            d_read[k].swap(fresh[k]);
            d_rep[k].swap(fresh[2 + k]);
        }
        cur = 0;
    }
    d_hash.room(stream, n_src, "the reads' hashes");
    d_slot.room(stream, n_src, "the reads' slots");
    d_words.room(stream, (n_src + 63) / 64, "the representatives' bitmap");
    d_table.room(stream, slots, "the table");
    d_ctr.room(stream, 2, "the counters");
    // ---- room: dst's, as take_reads makes it ----
    dst.compact_room(compact_tiles(n_src));
    uint64_t* result = dst.d_compact.p;
    uint64_t *tile_cnt = dst.d_compact.p + 3, *tile_bases = dst.d_compact.p + 3 + dst.compact_cap();
    uint32_t *new_read = d_read[cur ^ 1].p, *new_rep = d_rep[cur ^ 1].p;
    // ---- which reads are identical ----
    // (a batch as uploaded is normalised into the source's d_codes first, as run() would do it)
    if (!codes && nb_src) launch_normalise(stream, src.d_bases.p, src.d_codes.p, 0, nb_src);
    HIP_CHECK(hipMemsetAsync(result, 0, 3 * sizeof(uint64_t), stream));
    HIP_CHECK(hipMemsetAsync(d_ctr.p, 0, 2 * sizeof(uint64_t), stream));
    HIP_CHECK(hipMemsetAsync(d_words.p, 0, std::max<uint64_t>((n_src + 63) / 64, 1) * sizeof(uint64_t), stream));
    HIP_CHECK(hipEventRecord(ev[0], stream));
    launch_dedup_hash(stream, (uint32_t)n_src, s_off, s_codes, d_hash.p);
    HIP_CHECK(hipEventRecord(ev[1], stream));
    HIP_CHECK(hipMemsetAsync(d_table.p, 0xff, slots * sizeof(uint64_t), stream));
    launch_dedup_insert(stream, (uint32_t)n_src, s_off, s_codes, d_hash.p, hash_bits, d_table.p, (uint32_t)slots, d_slot.p, d_ctr.p);
    HIP_CHECK(hipEventRecord(ev[2], stream));
    launch_dedup_resolve(stream, (uint32_t)n_src, d_table.p, d_slot.p, s_map, d_words.p, new_read, new_rep, d_ctr.p);
    HIP_CHECK(hipEventRecord(ev[3], stream));
    // ---- the representatives, packed by the kernels of take_reads (bitmap, keep = set) ----
    launch_compact_scan(stream, (uint32_t)n_src, d_words.p, s_off, MTSV_KEEP_MATCHED, tile_cnt, tile_bases, result);
    HIP_CHECK(hipEventRecord(ev[4], stream));
    uint64_t h_result[3] = {0, 0, 0}, h_ctr[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(h_result, result, sizeof h_result, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(h_ctr, d_ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    const uint64_t m = h_result[0], nb = h_result[1];
    if (h_ctr[1]) throw std::runtime_error("internal: " + std::to_string(h_ctr[1]) + " reads found no slot in a table of " + std::to_string(slots) + " for " + std::to_string(n_src) + " reads");
    if (h_ctr[0] != m || m > n_src || (n_src && !m))
        throw std::runtime_error("internal: " + std::to_string(h_ctr[0]) + " representatives counted, " + std::to_string(m) + " scanned, of " + std::to_string(n_src) + " reads");
    if (m > dst.max_reads || nb > dst.max_bases)
        throw std::runtime_error("arg: " + std::to_string(m) + " distinct reads of " + std::to_string(nb) + " bases, the destination workspace was created for " +
                                 std::to_string(dst.max_reads) + " reads of " + std::to_string(dst.max_bases) + " bases");
    // from here on the destination's resident batch is being replaced
    dst.resident = false;
    dst.last_run = Batch::kRunNone;
    HIP_CHECK(hipEventRecord(ev[5], stream));
    launch_compact_copy(stream, (uint32_t)n_src, d_words.p, s_off, s_codes, MTSV_KEEP_MATCHED, s_map, tile_cnt, tile_bases, result, dst.d_codes.p, dst.d_read_off.p,
                        dst.d_read_map.p);
    HIP_CHECK(hipEventRecord(ev[6], stream));
    dst.h_read_off.resize(m + 1);
    HIP_CHECK(hipMemcpyAsync(dst.h_read_off.data(), dst.d_read_off.p, (m + 1) * 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (dst.h_read_off[0] != 0 || dst.h_read_off[m] != nb) throw std::runtime_error("internal: offsets of the distinct reads do not close on their bases");
    HIP_CHECK(hipEventElapsedTime(&ms_hash, ev[0], ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms_insert, ev[1], ev[2]));
    HIP_CHECK(hipEventElapsedTime(&ms_resolve, ev[2], ev[3]));
    HIP_CHECK(hipEventElapsedTime(&ms_scan, ev[3], ev[4]));
    HIP_CHECK(hipEventElapsedTime(&ms_copy, ev[5], ev[6]));
    dst.n_reads = m;
    dst.max_len = (uint32_t)h_result[2];
    dst.n_hits_total = 0;
    dst.total_hits = 0;
    dst.segments.clear();
    dst.resident = dst.codes_resident = dst.mapped = true;
    cur ^= 1;
    valid = true;
    n = n_src;
    n_unique = m;
    *n_unique_out = m;
    *bases_kept = nb;
    if (device_ms) *device_ms = ms_hash + ms_insert + ms_resolve + ms_scan + ms_copy;
    if (trace)
        fprintf(stderr,
                "[dedup] %llu of %llu reads distinct, %llu bases; hash %.3f ms, insert %.3f ms (%llu slots, %u hash bits), resolve %.3f ms, scan %.3f ms, copy %.3f ms; "
                "%llu bytes to the host, 0 to the device\n",
                (unsigned long long)m, (unsigned long long)n_src, (unsigned long long)nb, ms_hash, ms_insert, (unsigned long long)slots, hash_bits, ms_resolve, ms_scan,
                ms_copy, (unsigned long long)(sizeof h_result + sizeof h_ctr + (m + 1) * 4));
}

void DupMap::download(std::vector<uint64_t>& read, std::vector<uint64_t>& rep) const {
    read.clear();
    rep.clear();
    if (!valid || !n) return;
    std::vector<uint32_t> a(n), b(n);
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipMemcpy(a.data(), d_read[cur].p, n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(b.data(), d_rep[cur].p, n * 4, hipMemcpyDeviceToHost));
    read.assign(a.begin(), a.end());
    rep.assign(b.begin(), b.end());
}

// ---------------------------------------------------------------------------------------------
// The fan: dst := the records src holds for the representatives, once per read they stand for.  Count and scan first; the
// host reads the total and the records that belong to representatives (16 bytes) and refuses before anything is written.
// The records go into dst's other array, or a new pair when it is too small, which dst takes only when all is done.
// ---------------------------------------------------------------------------------------------
void DupMap::expand(Fold& dst, Fold& src, float* device_ms) const {
    if (&dst == &src) throw std::runtime_error("arg: the output fold is the fold itself");
    if (dst.grain != src.grain) throw std::runtime_error("arg: the output fold's grain is " + std::to_string(dst.grain) + ", the fold's " + std::to_string(src.grain));
    if (dst.device != src.device) throw std::runtime_error("arg: the output fold is on device " + std::to_string(dst.device) + ", the fold on device " + std::to_string(src.device));
    if (device != src.device) throw std::runtime_error("arg: the map is on device " + std::to_string(device) + ", the folds on device " + std::to_string(src.device));
    if (!valid) throw std::runtime_error("arg: the map holds no take (mtsv_batch_take_unique)");
    if (device_ms) *device_ms = 0;
    if (!src.n || !n) {
        if (src.n) throw std::runtime_error("arg: the fold holds " + std::to_string(src.n) + " records, the map no read");
        dst.reset(src.n_reads);
        dst.taxa = src.taxa;
        return;
    }
    HIP_CHECK(hipSetDevice(device));
    hipStream_t stream = dst.stream;
    Fan& f = fan;
    f.d_first.room(stream, n, "the reads' first records");
    f.d_cnt.room(stream, n, "the reads' record counts");
    f.d_off.room(stream, n + 1, "the reads' offsets");
    f.d_sums.room(stream, (uint64_t)scan_tiles((uint32_t)n) + 3, "the scan's sums");
    f.sums_cap = f.d_sums.cap - 2;  // (the total and the counter lie behind the sums)
    const uint32_t *rd = d_read[cur].p, *rp = d_rep[cur].p;
    uint64_t *d_total = f.d_sums.p + f.sums_cap, *d_own = d_total + 1;
    HIP_CHECK(hipMemsetAsync(d_total, 0, 2 * sizeof(uint64_t), stream));
    HIP_CHECK(hipEventRecord(f.ev[0], stream));
    launch_fan_count(stream, src.grain, (uint32_t)n, rd, rp, src.d_rec[src.cur].p, (uint32_t)src.n, f.d_first.p, f.d_cnt.p, d_own);
    launch_scan(stream, f.d_cnt.p, (uint32_t)n, f.d_sums.p, d_total, f.d_off.p);
    HIP_CHECK(hipEventRecord(f.ev[1], stream));
    uint64_t h[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(h, d_total, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    const uint64_t total = h[0], own = h[1];
    if (own != src.n)
        throw std::runtime_error("arg: " + std::to_string(src.n - std::min(own, src.n)) + " of the fold's " + std::to_string(src.n) +
                                 " records belong to reads that are no representatives in the map");
    if (total >= (1ull << 32)) throw std::runtime_error("limit: the expanded fold would hold " + std::to_string(total) + " records, 2^32 or more");
    if (total < own) throw std::runtime_error("internal: " + std::to_string(own) + " records of representatives, " + std::to_string(total) + " after the fan");
    Fold::Staged st = dst.stage_write(total, "an output fold");  // (an error below frees a pair it holds: dst stays as it was)
    float ms_count = 0, ms_write = 0;
    std::vector<uint32_t> taxa = src.taxa;
    HIP_CHECK(hipEventRecord(f.ev[2], stream));
    launch_fan_write(stream, src.grain, (uint32_t)n, rd, f.d_first.p, f.d_off.p, src.d_rec[src.cur].p, fan_tile, (uint32_t)total, st.dst);
    HIP_CHECK(hipEventRecord(f.ev[3], stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventElapsedTime(&ms_count, f.ev[0], f.ev[1]));
    HIP_CHECK(hipEventElapsedTime(&ms_write, f.ev[2], f.ev[3]));
    // ---- nothing can fail from here ----
    dst.commit(st, total);
    dst.n_reads = src.n_reads;
    dst.taxa.swap(taxa);
    if (device_ms) *device_ms = ms_count + ms_write;
    if (trace)
        fprintf(stderr, "[expand] %llu records of %llu representatives -> %llu records of %llu reads in tiles of %u: count and scan %.3f ms, write %.3f ms\n",
                (unsigned long long)src.n, (unsigned long long)n_unique, (unsigned long long)total, (unsigned long long)n, fan_tile, ms_count, ms_write);
}

}  // namespace mtsv
