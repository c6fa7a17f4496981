// binner_ingest.cpp -- see binner_ingest.hpp
#include "binner_ingest.hpp"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "binner_handles.hpp"

namespace mtsv_cli {

std::unique_ptr<ReadBlock> BlockPool::get() {
    std::lock_guard<std::mutex> lk(mu_);
    if (free_.empty()) return std::make_unique<ReadBlock>();
    auto b = std::move(free_.back());
    free_.pop_back();
    b->clear();
    return b;
}
void BlockPool::put(std::unique_ptr<ReadBlock> b) {
    std::lock_guard<std::mutex> lk(mu_);
    if (free_.size() < keep_) free_.push_back(std::move(b));
}
void BlockPool::stock(size_t n, uint64_t base_bytes) {
    std::vector<std::thread> th;
    std::vector<std::unique_ptr<ReadBlock>> made(n);
    for (size_t k = 0; k < n; k++)
        th.emplace_back([&made, k, base_bytes] {
            made[k] = std::make_unique<ReadBlock>();
            made[k]->bases.reserve(base_bytes);
        });
    for (auto& t : th) t.join();
    std::lock_guard<std::mutex> lk(mu_);
    keep_ = std::max(keep_, n);
    for (auto& b : made) free_.push_back(std::move(b));
}

bool install_pinned_blocks(uint64_t batch_reads) {
    if (getenv("MTSV_CLI_PAGEABLE") || batch_reads * 320 > (128ull << 20)) return false;
    mtsv_ingest::byte_alloc().alloc = [](size_t n) { return mtsv_host_alloc(n); };
    mtsv_ingest::byte_alloc().release = [](void* q) { mtsv_host_free(q); };
    return true;
}

InputHead sniff_head(const std::string& input, bool fastq) {
    InputHead h;
    FILE* hf = fopen(input.c_str(), "rb");
    if (!hf) return h;
    std::vector<char> head(256 << 10);
    const size_t got = fread(head.data(), 1, head.size(), hf);
    fclose(hf);
    if (got < 2 || ((uint8_t)head[0] == 0x1f && (uint8_t)head[1] == 0x8b)) return h;
    uint64_t recs = 0;
    if (fastq) {
        uint64_t lines = 0;
        for (size_t i = 0; i < got; i++) lines += head[i] == '\n';
        recs = lines / 4;
    } else {
        for (size_t i = 0; i < got; i++) recs += head[i] == '>' && (i == 0 || head[i - 1] == '\n');
    }
    if (recs >= 8) h.bytes_per_record = (double)got / (double)recs;
    const char* end = head.data() + std::min<size_t>(got, 64 << 10);
    if (const char* nl = (const char*)memchr(head.data(), '\n', (size_t)(end - head.data())))
        for (const char* q = nl + 1; q < end && *q != '>' && *q != '+'; q++) h.first_read_len += *q != '\n' && *q != '\r';
    return h;
}

bool Producer::open() {
    rd_.fastq = run_.fastq;
    if (!rd_.in.open(run_.input)) return false;
    head_ = sniff_head(run_.input, run_.fastq);
    return true;
}

// Plain input is cut into blocks of about one batch of reads each (bytes per record estimated from the file's
// head): a parsed block then IS the batch -- its bases lie in page-locked memory (byte_alloc) that the copy
// engine reads in place, and the producer thread hands it on without touching the bases again.
uint64_t Producer::ingest_block_bytes(uint64_t batch_reads) const {
    if (const char* e = getenv("MTSV_INGEST_BLOCK")) return strtoull(e, nullptr, 10);
    if (head_.bytes_per_record == 0) return 16ull << 20;
    // (capped at 96 MiB: a parser thread is slower per byte on larger blocks -- 1 Mi-read blocks of 335 MB parsed at a
    //  third of the rate -- and batches beyond that are put together from several blocks as before)
    return std::min<uint64_t>(std::max<uint64_t>((uint64_t)(head_.bytes_per_record * (double)batch_reads), 4ull << 20), 96ull << 20);
}

static bool is_full(const ReadBlock& w, uint64_t batch_reads) { return w.n() >= batch_reads || w.bases.size() >= (1ull << 30); }

bool Producer::produce(uint64_t batch_reads, const Emit& emit) {
    const uint64_t read_offset = run_.read_offset;
    auto w = pool.get();
    uint64_t skipped = 0;
    if (getenv("MTSV_SERIAL_INGEST")) return produce_serial(std::move(w), skipped, batch_reads, emit);
    mtsv_ingest::ParallelFastx par;
    mtsv_ingest::GzFastx gzpar;  // gzip input: parallel inflate + the same block parsers (MTSV_SERIAL_GZIP=1: zlib's one stream)
    // inflating is the expensive part of gzip input: more helpers than plain text needs (measured: 8 threads 3.3 M
    // reads/s, 16 5.5, 32 5.7 against 1.3 on zlib's one stream)
    // (-t / --threads bounds it like every other host-side pool; MTSV_GZ_THREADS=16 is what the 9.0 M reads/s were measured with)
    unsigned gz_threads = run_.host_threads;
    if (const char* e = getenv("MTSV_GZ_THREADS")) gz_threads = (unsigned)std::max(1, atoi(e));
    gz_threads = std::min(gz_threads, std::max(1u, std::thread::hardware_concurrency()));
    const uint64_t ingest_block = ingest_block_bytes(batch_reads);
    par.prepare = [this](ReadBlock& b) {
        auto stocked = pool.get();
        std::swap(b, *stocked);
    };
    bool use_gz = false;
    if (!par.open(run_.input, run_.fastq, run_.host_threads, ingest_block)) {
        if (getenv("MTSV_SERIAL_GZIP") || !gzpar.open(run_.input, run_.fastq, gz_threads, ingest_block))
            return produce_serial(std::move(w), skipped, batch_reads, emit);
        use_gz = true;
    }
    auto blk_owner = pool.get();
    uint64_t irregular = 0, direct_emitted = 0;
    for (;;) {
        ReadBlock& blk = *blk_owner;
        auto r = use_gz ? gzpar.next(blk, &irregular) : par.next(blk, &irregular);
        if (r == mtsv_ingest::ParallelFastx::END) break;
        if (r == mtsv_ingest::ParallelFastx::CORRUPT) {  // records of a member whose CRC-32 then failed have been handed out
            rd_.fail("corrupt gzip data (CRC mismatch)");
            return false;
        }
        if (r == mtsv_ingest::ParallelFastx::IRREGULAR) {
            logmsg("DEBUG", std::string(use_gz ? "gzip input" : "input") + " is not plain 4-line FASTQ / FASTA (or not decodable in parallel) at byte " + std::to_string(irregular) + "; continuing with the serial reader");
            if (gzseek(rd_.in.f, (z_off_t)irregular, SEEK_SET) < 0) {
                rd_.fail("read error");
                return false;
            }
            par.close();
            gzpar.close();
            return produce_serial(std::move(w), skipped, batch_reads, emit);  // continues from here
        }
        uint64_t from = 0;
        if (skipped < read_offset) {
            from = std::min<uint64_t>(read_offset - skipped, blk.n());
            skipped += from;
        }
        // a block of about a batch, nothing pending: the block is the batch
        // (smaller blocks are collected into a batch -- except the first ones of the file, which the parser cuts
        //  short on purpose so that the GPU has work early)
        if (from == 0 && w->n() == 0 && blk.n() && blk.n() <= block_reads_max(batch_reads) && blk.bases.size() < (1ull << 30) &&
            (2 * blk.n() >= batch_reads || direct_emitted < 4)) {
            direct_emitted++;
            if (!emit(std::move(blk_owner))) return true;
            blk_owner = pool.get();
            continue;
        }
        // cut the block at batch boundaries
        while (from < blk.n()) {
            const uint64_t room = batch_reads > w->n() ? batch_reads - w->n() : 0;
            const uint64_t take = std::min<uint64_t>(room, blk.n() - from);
            w->append(blk, from, from + take);  // records [from, from + take)
            from += take;
            if (is_full(*w, batch_reads)) {
                if (!emit(std::move(w))) return true;
                w = pool.get();
            }
        }
    }
    if (w->n() && !emit(std::move(w))) return true;
    if (all_emitted) all_emitted();  // before the teardown: unmapping a 10 GB input took 45 ms
    par.close();
    gzpar.close();
    return true;
}

// the serial reader, from where it stands: the start of the input, or the first block the parallel parsers handed back
bool Producer::produce_serial(std::unique_ptr<ReadBlock> w, uint64_t skipped, uint64_t batch_reads, const Emit& emit) {
    mtsv_ingest::Record r;
    while (rd_.next(r)) {
        if (skipped < run_.read_offset) {
            skipped++;
            continue;
        }
        mtsv_ingest::push_record(*w, r);
        if (is_full(*w, batch_reads)) {
            if (!emit(std::move(w))) return true;
            w = pool.get();
        }
    }
    if (rd_.error) return false;
    if (w->n()) emit(std::move(w));
    if (all_emitted) all_emitted();
    return true;
}

int parse_only(const Run& run, Producer& producer) {
    uint64_t n = 0, nb = 0, hb = 1469598103934665603ull, hi = 1469598103934665603ull, hl = 1469598103934665603ull;
    auto fnv = [](uint64_t& h, const uint8_t* p, uint64_t len) {
        for (uint64_t i = 0; i < len; i++) h = (h ^ p[i]) * 1099511628211ull;
    };
    const bool ok = producer.produce(run.batch_reads, [&](std::unique_ptr<ReadBlock> w) {
        n += w->n();
        nb += w->bases.size();
        if (getenv("MTSV_PARSE_NOHASH")) {
            producer.pool.put(std::move(w));
            return true;
        }
        fnv(hb, w->bases.data(), w->bases.size());
        fnv(hi, (const uint8_t*)w->ids.data(), w->ids.size());
        for (uint64_t r = 0; r < w->n(); r++) {
            uint64_t len = w->off[r + 1] - w->off[r];
            fnv(hl, (const uint8_t*)&len, 8);
        }
        return true;
    });
    if (!ok) {
        logmsg("ERROR", "Unable to read from input file: " + producer.error());
        return 12;
    }
    printf("records=%llu bases=%llu bases_fnv=%016llx ids_fnv=%016llx lens_fnv=%016llx\n", (unsigned long long)n,
           (unsigned long long)nb, (unsigned long long)hb, (unsigned long long)hi, (unsigned long long)hl);
    return 0;
}

}  // namespace mtsv_cli
