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

namespace {
template <class T>
T* dedup_alloc(uint64_t count) {
    T* p = nullptr;
    HIP_CHECK(hipMalloc((void**)&p, std::max<uint64_t>(count, 1) * sizeof(T)));
    return p;
}
template <class T>
void dedup_free(T*& p) {
    if (p) (void)hipFree(p);
    p = nullptr;
}
}  // namespace

DupMap::DupMap(int device_) : device(device_) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess) {
        (void)hipGetLastError();
        n_dev = 0;
    }
    if (device < 0 || device >= n_dev) throw std::runtime_error("device: no HIP device " + std::to_string(device) + " (" + std::to_string(n_dev) + " visible)");
    if (const char* e = getenv("MTSV_DEDUP_HASH_BITS")) hash_bits = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), 64);  // (tests: long chains, equal tags)
    if (const char* e = getenv("MTSV_FAN_TILE")) {  // (tests: tile edges within reach of small lists)
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 10), 64), kFanTileMax);
        fan_tile = 64;
        while (fan_tile * 2 <= want) fan_tile *= 2;
    }
    trace = getenv("MTSV_TRACE") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    for (auto& e : ev) HIP_CHECK(hipEventCreate(&e));
    for (auto& e : fan.ev) HIP_CHECK(hipEventCreate(&e));
}

DupMap::~DupMap() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    for (void* p : {(void*)d_read[0], (void*)d_read[1], (void*)d_rep[0], (void*)d_rep[1], (void*)d_hash, (void*)d_table, (void*)d_words, (void*)d_ctr,
                    (void*)d_slot, (void*)fan.d_first, (void*)fan.d_cnt, (void*)fan.d_off, (void*)fan.d_sums})
        if (p) (void)hipFree(p);
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : fan.ev)
        if (e) (void)hipEventDestroy(e);
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
    const uint32_t* ho = host_batch ? src.h_off_all : src.h_read_off.data();
    const uint64_t nb_src = n_src ? ho[n_src] : 0;
    const bool codes = host_batch || src.codes_resident;
    const uint8_t* s_codes = host_batch ? src.arena[0].d_bases : src.d_codes;
    const uint32_t* s_off = host_batch ? src.arena[0].d_off : src.d_read_off;
    const uint32_t* s_map = !host_batch && src.mapped ? src.d_read_map : nullptr;
    HIP_CHECK(hipSetDevice(device));
    hipStream_t stream = dst.stream;
    // ---- room: the map's (a refusal from here on leaves both the map and dst as they were) ----
    uint64_t slots = 2;
    while (slots < 2 * n_src) slots *= 2;
    if (n_src > cap || !d_read[0]) {
        const uint64_t ncap = std::max<uint64_t>(n_src + n_src / 8, 1024);
        uint32_t* a[4] = {nullptr, nullptr, nullptr, nullptr};
        try {
            for (auto& p : a) p = dedup_alloc<uint32_t>(ncap);
            if (valid && n) {
                HIP_CHECK(hipMemcpyAsync(a[0], d_read[cur], n * 4, hipMemcpyDeviceToDevice, stream));
                HIP_CHECK(hipMemcpyAsync(a[2], d_rep[cur], n * 4, hipMemcpyDeviceToDevice, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
            }
        } catch (...) {
            for (auto& p : a) dedup_free(p);
            throw;
        }
        for (int k = 0; k < 2; k++) {
            dedup_free(d_read[k]);
            dedup_free(d_rep[k]);
        }
        d_read[0] = a[0];
        d_read[1] = a[1];
        d_rep[0] = a[2];
        d_rep[1] = a[3];
        cur = 0;
        cap = ncap;
    }
    if (n_src > reads_cap || !d_hash) {
        const uint64_t ncap = std::max<uint64_t>(n_src + n_src / 8, 1024);
        dedup_free(d_hash);
        dedup_free(d_slot);
        dedup_free(d_words);
        reads_cap = 0;
        d_hash = dedup_alloc<uint64_t>(ncap);
        d_slot = dedup_alloc<uint32_t>(ncap);
        d_words = dedup_alloc<uint64_t>((ncap + 63) / 64);
        reads_cap = ncap;
    }
    if (slots > table_cap || !d_table) {
        dedup_free(d_table);
        table_cap = 0;
        d_table = dedup_alloc<uint64_t>(slots);
        table_cap = slots;
    }
    if (!d_ctr) d_ctr = dedup_alloc<uint64_t>(2);
    // ---- room: dst's, as take_reads makes it ----
    const uint64_t tiles = compact_tiles(n_src);
    if (!dst.d_compact || dst.compact_cap < tiles) {
        (void)hipFree(dst.d_compact);
        dst.d_compact = nullptr;
        dst.compact_cap = 0;
        dst.d_compact = dedup_alloc<uint64_t>(3 + 2 * (tiles + tiles / 16));
        dst.compact_cap = tiles + tiles / 16;
    }
    if (!dst.d_read_map) dst.d_read_map = dedup_alloc<uint32_t>(dst.max_reads);
    uint64_t* result = dst.d_compact;
    uint64_t *tile_cnt = dst.d_compact + 3, *tile_bases = dst.d_compact + 3 + dst.compact_cap;
    uint32_t *new_read = d_read[cur ^ 1], *new_rep = d_rep[cur ^ 1];
    // ---- which reads are identical ----
    // (a batch as uploaded is normalised into the source's d_codes first, as run() would do it)
    if (!codes && nb_src) launch_normalise(stream, src.d_bases, src.d_codes, 0, nb_src);
    HIP_CHECK(hipMemsetAsync(result, 0, 3 * sizeof(uint64_t), stream));
    HIP_CHECK(hipMemsetAsync(d_ctr, 0, 2 * sizeof(uint64_t), stream));
    HIP_CHECK(hipMemsetAsync(d_words, 0, std::max<uint64_t>((n_src + 63) / 64, 1) * sizeof(uint64_t), stream));
    HIP_CHECK(hipEventRecord(ev[0], stream));
    launch_dedup_hash(stream, (uint32_t)n_src, s_off, s_codes, d_hash);
    HIP_CHECK(hipEventRecord(ev[1], stream));
    HIP_CHECK(hipMemsetAsync(d_table, 0xff, slots * sizeof(uint64_t), stream));
    launch_dedup_insert(stream, (uint32_t)n_src, s_off, s_codes, d_hash, hash_bits, d_table, (uint32_t)slots, d_slot, d_ctr);
    HIP_CHECK(hipEventRecord(ev[2], stream));
    launch_dedup_resolve(stream, (uint32_t)n_src, d_table, d_slot, s_map, d_words, new_read, new_rep, d_ctr);
    HIP_CHECK(hipEventRecord(ev[3], stream));
    // ---- the representatives, packed by the kernels of take_reads (bitmap, keep = set) ----
    launch_compact_scan(stream, (uint32_t)n_src, d_words, s_off, MTSV_KEEP_MATCHED, tile_cnt, tile_bases, result);
    HIP_CHECK(hipEventRecord(ev[4], stream));
    uint64_t h_result[3] = {0, 0, 0}, h_ctr[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(h_result, result, sizeof h_result, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(h_ctr, d_ctr, sizeof h_ctr, hipMemcpyDeviceToHost, stream));
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
    launch_compact_copy(stream, (uint32_t)n_src, d_words, s_off, s_codes, MTSV_KEEP_MATCHED, s_map, tile_cnt, tile_bases, result, dst.d_codes, dst.d_read_off,
                        dst.d_read_map);
    HIP_CHECK(hipEventRecord(ev[6], stream));
    dst.h_read_off.resize(m + 1);
    HIP_CHECK(hipMemcpyAsync(dst.h_read_off.data(), dst.d_read_off, (m + 1) * 4, hipMemcpyDeviceToHost, stream));
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
    HIP_CHECK(hipMemcpy(a.data(), d_read[cur], n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(b.data(), d_rep[cur], n * 4, hipMemcpyDeviceToHost));
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
    if (n > f.cap || !f.d_first) {
        const uint64_t ncap = std::max<uint64_t>(n + n / 8, 1024);
        dedup_free(f.d_first);
        dedup_free(f.d_cnt);
        dedup_free(f.d_off);
        dedup_free(f.d_sums);
        f.cap = 0;
        f.d_first = dedup_alloc<uint32_t>(ncap);
        f.d_cnt = dedup_alloc<uint32_t>(ncap);
        f.d_off = dedup_alloc<uint32_t>(ncap + 1);
        f.sums_cap = (uint64_t)scan_tiles((uint32_t)ncap) + 1;
        f.d_sums = dedup_alloc<uint64_t>(f.sums_cap + 2);
        f.cap = ncap;
    }
    const uint32_t *rd = d_read[cur], *rp = d_rep[cur];
    uint64_t *d_total = f.d_sums + f.sums_cap, *d_own = d_total + 1;
    const uint64_t rec = src.rec_bytes();
    HIP_CHECK(hipMemsetAsync(d_total, 0, 2 * sizeof(uint64_t), stream));
    HIP_CHECK(hipEventRecord(f.ev[0], stream));
    launch_fan_count(stream, src.grain, (uint32_t)n, rd, rp, src.d_rec[src.cur], (uint32_t)src.n, f.d_first, f.d_cnt, d_own);
    launch_scan(stream, f.d_cnt, (uint32_t)n, f.d_sums, d_total, f.d_off);
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
    uint8_t *grown_a = nullptr, *grown_b = nullptr, *out = nullptr;
    uint64_t grown_cap = 0;
    if (total > dst.cap || !dst.d_rec[0]) {
        grown_cap = std::min<uint64_t>(std::max<uint64_t>(total, 1ull << 16), 0xffffffffull);
        const bool ok_a = hipMalloc((void**)&grown_a, grown_cap * rec) == hipSuccess;
        const bool ok_b = ok_a && hipMalloc((void**)&grown_b, grown_cap * rec) == hipSuccess;
        if (!ok_b) {
            (void)hipGetLastError();
            if (grown_a) (void)hipFree(grown_a);
            throw std::runtime_error("device: no memory for an output fold of " + std::to_string(grown_cap) + " records (two arrays)");
        }
        out = grown_a;
    } else {
        out = dst.d_rec[dst.cur ^ 1];
    }
    float ms_count = 0, ms_write = 0;
    std::vector<uint32_t> taxa;
    try {
        taxa = src.taxa;
        HIP_CHECK(hipEventRecord(f.ev[2], stream));
        launch_fan_write(stream, src.grain, (uint32_t)n, rd, f.d_first, f.d_off, src.d_rec[src.cur], fan_tile, (uint32_t)total, out);
        HIP_CHECK(hipEventRecord(f.ev[3], stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&ms_count, f.ev[0], f.ev[1]));
        HIP_CHECK(hipEventElapsedTime(&ms_write, f.ev[2], f.ev[3]));
    } catch (...) {
        if (grown_a) (void)hipFree(grown_a);
        if (grown_b) (void)hipFree(grown_b);
        throw;
    }
    // ---- nothing can fail from here ----
    if (grown_a) {
        if (dst.d_rec[0]) (void)hipFree(dst.d_rec[0]);
        if (dst.d_rec[1]) (void)hipFree(dst.d_rec[1]);
        dst.d_rec[0] = grown_a;
        dst.d_rec[1] = grown_b;
        dst.cur = 0;
        dst.cap = grown_cap;
    } else {
        dst.cur ^= 1;
    }
    dst.n = total;
    dst.n_reads = src.n_reads;
    dst.taxa.swap(taxa);
    if (device_ms) *device_ms = ms_count + ms_write;
    if (trace)
        fprintf(stderr, "[expand] %llu records of %llu representatives -> %llu records of %llu reads in tiles of %u: count and scan %.3f ms, write %.3f ms\n",
                (unsigned long long)src.n, (unsigned long long)n_unique, (unsigned long long)total, (unsigned long long)n, fan_tile, ms_count, ms_write);
}

}  // namespace mtsv
