// batch_host.hip -- the run of a batch that lies in host memory (Batch::run_host, run_host_parts): what it sizes by the
// batch, and Batch::HostRun, the run's shared state and the jobs of its threads.  The feeder's arithmetic is host_feed.hpp,
// the lanes' range_take is pass_plan.hpp; the pinned arrays the results leave in are PinnedStage (batch.hpp, batch.hip).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <thread>
#include <vector>

#include "batch.hpp"
#include "host_feed.hpp"

namespace mtsv {

namespace {
// memcpy / first-touch split over a few threads for large host buffers
template <class F>
void parallel_ranges(uint64_t n, F f) {
    static const int max_nt = [] {
        const char* e = getenv("MTSV_COPY_THREADS");
        return e ? std::max(1, std::min(16, atoi(e))) : 4;
    }();
    const int nt = std::min(max_nt, n >= (32ull << 20) ? 4 : n >= (4ull << 20) ? 2 : 1);
    if (nt == 1) return f(0, n);
    std::vector<std::thread> th;
    const uint64_t chunk = ((n + nt - 1) / nt + 4095) & ~4095ull;
    for (int k = 0; k < nt; k++) {
        uint64_t a = std::min(n, chunk * k), b = std::min(n, chunk * (k + 1));
        if (a < b) th.emplace_back([=] { f(a, b); });
    }
    for (auto& t : th) t.join();
}
void parallel_copy(uint8_t* dst, const uint8_t* src, uint64_t n) {
    parallel_ranges(n, [=](uint64_t a, uint64_t b) { memcpy(dst + a, src + a, b - a); });
}

constexpr uint64_t kChunkMax = 32ull << 20, kChunkMin = 4ull << 20;  // bases of a copy chunk: the first, doubling up to the largest

// One host batch at a time has the packer: a second one that runs beside it in this process -- another device of
// mtsv_bin_batch_multi, another worker -- would wait for the pool chunk by chunk, and sends its bytes plain.
std::atomic<int> host_runs{0};
struct PackerClaim {
    const int mine;
    PackerClaim() : mine(++host_runs) {}
    ~PackerClaim() { host_runs--; }
    bool first() const { return mine == 1; }
};

// threads that are joined on every way out of the scope
struct JoinedThreads {
    std::vector<std::thread> th;
    ~JoinedThreads() {
        for (auto& t : th) t.join();
    }
};
// Batch::commit_mu names the run's mutex for as long as the scope lasts
struct CommitMutexScope {
    std::mutex*& slot;
    CommitMutexScope(std::mutex*& slot_, std::mutex& mu) : slot(slot_) { slot = &mu; }
    ~CommitMutexScope() { slot = nullptr; }
};
}  // namespace

// Host buffers in, hits in pinned host memory out.
//
// The PCIe rate of the reads (~50 GB/s = 330 k reads of 150 bases per ms) and the rate of the kernels are about
// equal, so the copy must run flat out from the first microsecond and the kernels must follow right behind it:
//   * one FEEDER thread copies the batch, strictly in read order, in chunks of a few MB (growing to 32 MB) on one
//     copy stream into an ARENA in HBM that holds the whole batch (or 3 GiB segments of it, two arenas taking
//     turns), an event after every chunk.  Bases in page-locked memory are copied from where they lie, others are
//     staged through a few page-locked chunk buffers; the u64 offsets are narrowed to arena-relative u32 on the way;
//   * the LANES -- a host thread and a stream each -- take the reads that HAVE ARRIVED and nobody has taken yet:
//     a pass is a range of reads of the arena, as large as the ramp allows and the copy has delivered, never
//     tied to how the copy was cut.  An idle device takes what is there; while other lanes keep it busy a lane
//     waits for a worthwhile range (the ramp grows with the reads already taken and falls towards the end, so
//     the lanes finish together);
//   * a finished range's hits leave for the pinned result array at once, in read order, on a third stream.
// ---------------------------------------------------------------------------------------------
void Batch::run_host(const uint8_t* bases, const uint64_t* read_off, uint64_t n, const mtsv_params& p, uint64_t read_base) {
    const HostPart one{bases, read_off, n};
    run_host_parts(&one, 1, p, read_base);
}

// What run_host sizes by its batch: the copy streams, the device arenas, the page-locked offset table.
void Batch::host_room(uint64_t n, uint64_t total_bases, bool trace) {
    if (!copy_stream) {
        // The copy streams get a priority of their own.  The runtime maps streams onto a few hardware queues (four by
        // default, GPU_MAX_HW_QUEUES) round robin, per priority; an asynchronous copy holds its queue with a barrier
        // packet until the copy engine is done, and with it every kernel of any stream that shares the queue -- a lane
        // that shared one with the reads' transfer did not get a kernel in for 20 ms at a time.
        int prio_low = 0, prio_high = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
        copy_stream.create(hipStreamNonBlocking, prio_high);
        copy_stream2.create(hipStreamNonBlocking, prio_high);
    }
    uint64_t arena_bases = kArenaBases, arena_reads = kArenaReads;
    if (const char* e = getenv("MTSV_ARENA_BASES")) arena_bases = std::max<uint64_t>(1 << 16, strtoull(e, nullptr, 10));  // (tests)
    const bool one_segment = total_bases <= arena_bases && n <= arena_reads;
    {
        const uint64_t want_b = one_segment ? total_bases : arena_bases, want_r = one_segment ? n : std::min(n, arena_reads);
        for (int k = 0; k < (one_segment ? 1 : 2); k++) {
            Arena& ar = arena[k];
            if (ar.cap_bases < want_b || ar.cap_reads < want_r) {
                if (trace) fprintf(stderr, "[run_host] arena %d: %.1f MB of bases, %llu reads\n", k, want_b / 1e6, (unsigned long long)want_r);
                const uint64_t cb = want_b + want_b / 16, cr = want_r + want_r / 16;  // a little room: the next batch is rarely the same size
                ar.resize(k, std::min(cb, arena_bases), std::min(cr, arena_reads));
            }
        }
    }
    // the whole batch's narrowed offsets, every segment with a closing entry of its own (host_feed.hpp: off_index);
    // run_slice looks at read lengths on the host when a range holds long reads
    const uint64_t off_need = offsets_needed(n, total_bases, arena_bases, arena_reads, one_segment);
    if (h_off_all.cap < off_need) h_off_all.renew(off_need + n / 16);
}

void Batch::Arena::resize(int k, uint64_t bases, uint64_t reads) {
    cap_bases = cap_reads = 0;
    release_all(d_bases, d_packed, d_off);
    const std::string name = "arena " + std::to_string(k);
    d_bases.alloc(bases + 64, (name + ": bases").c_str());  // k_search reads up to 36 bytes past a seed start
    d_packed.alloc(bases / 2 + 64, (name + ": packed bases").c_str());
    d_off.alloc(reads + 1, (name + ": offsets").c_str());
    cap_bases = bases;
    cap_reads = reads;
}

void Batch::reserve_host(uint64_t n, uint64_t n_bases) {
    HIP_CHECK(hipSetDevice(di->device));
    host_room(n, n_bases, getenv("MTSV_TRACE") != nullptr);
    if (!keep_on_device) {  // a result array of the size the first call will ask for, parked in the pool
        uint64_t cap = 0;
        mtsv_hit* h = pinned_hits_alloc(n + n / 8, &cap);
        pinned_hits_release(h);
    }
}

// One host run: what its threads share, and one member function per job.  The feeder (feed) walks the batch with a
// FeedCursor and issues the copies; the watcher (watch) publishes what has arrived; every lane (lane_loop) takes ranges of
// arrived reads, runs them and commits what is finished, in read order.
struct Batch::HostRun {
    struct Chunk {
        uint64_t begin = 0, end = 0;  // reads
        uint32_t max_len = 0, seg = 0;
        hipEvent_t ev = nullptr;
    };
    struct Range {
        uint64_t begin = 0, end = 0;
        bool done = false;
        Batch* lane = nullptr;
        uint64_t hit_off = 0, hit_cnt = 0;
        uint64_t a_off = 0, a_cnt = 0;  // its assignments: they stay in the lane until mtsv_batch_download_assignments
    };
    struct Taken {  // a range a lane has taken: ranges[k], reads [rb, re) of segment seg, which begins at read seg_first
        uint64_t k = 0, rb = 0, re = 0, seg_first = 0;
        uint32_t seg = 0, ml = 0;
        uint64_t hit_off = 0, a_off = 0;  // where the lane's result arrays stood before it
    };

    // ---- fixed before the threads start ----
    Batch& b;
    const mtsv_params& p;
    const uint64_t read_base;
    const double t_entry = now_s();
    const bool trace = getenv("MTSV_TRACE") != nullptr;
    FeedView view;  // the parts as one batch
    uint64_t n = 0;
    std::vector<Batch*> lanes;
    std::optional<PackerClaim> packer;
    bool direct = false;  // every part is page-locked
    bool packed = false;  // the bases cross as 4-bit codes
    bool stage_hits = false, stage_assign = false;
    uint64_t a_rec = 0, n_lanes_used = 1, ramp_floor = 0, idle_take = 0;

    // ---- mu and what it protects: everything below, and of the workspace the two pinned stages, segments and max_len ----
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Chunk> chunks;            // issued copies, in read order
    std::vector<uint64_t> seg_begin{0};   // first read of every segment (feeder appends)
    uint64_t n_complete = 0;              // chunks [0, n_complete) have arrived
    bool issued_all = false;
    std::vector<Range> ranges;
    uint64_t next_read = 0;    // first read no lane has taken
    uint64_t next_commit = 0;  // next range whose hits go to the host
    uint64_t done_prefix = 0;  // reads [0, done_prefix) are through the kernels (arena reuse)
    int busy_lanes = 0;
    bool abort = false;
    std::exception_ptr first_err;

    HostRun(Batch& b_, const HostPart* parts, int n_parts, const mtsv_params& p_, uint64_t read_base_);
    void begin();
    void run_threads();
    void finish();

    void fail(std::exception_ptr e) {
        std::lock_guard<std::mutex> lk(mu);
        if (!first_err) first_err = e;
        abort = true;
        cv.notify_all();
    }
    void feed();
    bool open_segment(const FeedStep& s);
    uint32_t narrow_chunk(const FeedStep& s, const uint64_t* poff, uint32_t* ho);
    void copy_chunk(size_t k, const FeedStep& s, uint8_t& prev_code);
    void watch();
    void lane_loop(Batch* lane);
    bool take_range(Batch* lane, uint64_t last_done, Taken& t);
    void run_range_on_lane(Batch* lane, Taken& t);
    void finish_range(Batch* lane, const Taken& t);
    void commit_ready();
};

Batch::HostRun::HostRun(Batch& b_, const HostPart* parts, int n_parts, const mtsv_params& p_, uint64_t read_base_) : b(b_), p(p_), read_base(read_base_) {
    HIP_CHECK(hipSetDevice(b.di->device));
    lanes.push_back(&b);
    for (auto& l : b.extra) lanes.push_back(l.get());
    const bool stage_always = getenv("MTSV_STAGE_ALWAYS") != nullptr;
    for (int k = 0; k < n_parts; k++) {
        const HostPart& hp = parts[k];
        // bases in page-locked memory (mtsv_host_alloc / mtsv_host_register) go to the GPU from where they lie
        if (view.add(hp.bases, hp.read_off, hp.n))
            view.parts.back().pinned = host_pinned(hp.bases + hp.read_off[0], hp.read_off[hp.n] - hp.read_off[0]) && !stage_always;
    }
    n = view.n;
    issued_all = n == 0;
}

// begin_run, the room the batch needs, the transfer format, the pinned stages and how many lanes work
void Batch::HostRun::begin() {
    bool any_staged = false, any_direct = false;
    for (auto& v : view.parts) (v.pinned ? any_direct : any_staged) = true;
    direct = !any_staged;
    if (trace) fprintf(stderr, "[run_host] input %s%s\n", direct ? "page-locked: copied from the caller's buffer" : "pageable: staged",
                       any_staged && any_direct ? " (some parts page-locked)" : "");
    // ---- arenas: segments of at most kArenaBases bases / kArenaReads reads (u32 offsets inside a segment) ----
    b.host_room(n, view.total_bases, trace);
    // The bases cross PCIe as 4-bit codes, packed on the host chunk by chunk into page-locked staging buffers while the
    // chunk before is on its way -- when the process has the CPUs for it (host_pack.hpp).  Otherwise, and with
    // MTSV_H2D_PLAIN=1: the bytes as they are (from page-locked memory in place) and k_normalise on the device.
    packer.emplace();
    packed = !getenv("MTSV_H2D_PLAIN") && pack_threads() >= kPackWorthwhile && packer->first();
    if ((packed || !direct) && !b.h_stage[kStage - 1].p)
        for (auto& hs : b.h_stage)
            if (!hs.p) hs.renew(kChunkMax + 64);

    b.n_reads = n;
    b.max_len = 0;
    b.resident = b.codes_resident = b.mapped = false;  // (what upload() or take_reads() left is not this batch)
    if (trace) fprintf(stderr, "[run_host] entered; begin_run at %.2f ms\n", (now_s() - t_entry) * 1e3);
    b.begin_run(p, read_base);
    b.hits_stage.staged = 0;
    // (MTSV_ASSIGN_ONLY: the hits stay on the device, no hit byte crosses to the host; a pinned array left from an earlier
    //  run goes back to the pool)
    stage_hits = !b.keep_on_device && !b.assign_only();
    if (b.assign_only()) b.hits_stage.drop();
    // expect about as many hits as the last run produced (first run: one per read, and an eighth)
    if (stage_hits && !b.flags_only()) b.hits_stage.begin(n + n / 8);
    stage_assign = b.assign.mode != MTSV_ASSIGN_OFF;
    a_rec = b.assign.rec_bytes();
    if (stage_assign) b.assign_stage.begin(n + n / 8);
    if (trace) fprintf(stderr, "[run_host] result array of %llu hits ready at %.2f ms\n", (unsigned long long)b.hits_stage.cap, (now_s() - t_entry) * 1e3);
    n_lanes_used = n >= lanes.size() * kLaneMinReads ? lanes.size() : 1;
    b.lanes_used = n_lanes_used;
    // (the first ranges: with the bases packed the reads arrive faster than the device takes them, and fewer, larger ranges
    //  are worth more than an early start -- same-box medians 31.1-31.3 ms per step against 31.8-32.4 with 256 Ki; with the
    //  plain transfer the order is the other way round, 36.4 against 37.0)
    ramp_floor = packed ? 768 << 10 : 256 << 10;
    if (const char* e = getenv("MTSV_RAMP_FLOOR")) ramp_floor = std::max<uint64_t>(4096, strtoull(e, nullptr, 10));
    idle_take = 64 << 10;  // an idle device starts on this little
    if (const char* e = getenv("MTSV_IDLE_TAKE")) idle_take = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
}

// ---- feeder ----
void Batch::HostRun::feed() {
    try {
        HIP_CHECK(hipSetDevice(b.di->device));
        FeedCursor cur(view, b.arena[0].cap_bases, b.arena[0].cap_reads, b.arena[1].cap_bases, b.arena[1].cap_reads, kChunkMin, kChunkMax);
        uint8_t prev_code = 0;  // packed transfer: the code of the segment's last base so far (it may share a byte with the next)
        for (size_t k = 0; !cur.done();) {
            const FeedStep s = cur.next();
            if (s.kind == FeedStep::kLimit) throw std::runtime_error(s.limit_text());
            if (s.kind == FeedStep::kChunk) copy_chunk(k++, s, prev_code);
            else if (!open_segment(s)) return;
        }
    } catch (...) {
        fail(std::current_exception());
    }
}

// publishes the segment; false: the run has failed elsewhere
bool Batch::HostRun::open_segment(const FeedStep& s) {
    {
        std::lock_guard<std::mutex> lk(mu);
        seg_begin.push_back(s.r);
    }
    cv.notify_all();  // lanes waiting for more reads of the closed segment take what it has
    if (s.seg >= 2) {  // the arena's previous tenant (segment seg - 2) must be through the kernels
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return abort || done_prefix >= seg_begin[s.seg - 1]; });
        if (abort) return false;
    }
    return true;
}

// the chunk's offsets relative to its segment's first base, into its entries ho of the table; returns its longest read
uint32_t Batch::HostRun::narrow_chunk(const FeedStep& s, const uint64_t* poff, uint32_t* ho) {
    const uint64_t cnt = s.cnt();
    if (off_index(s.r, s.seg) + cnt + 1 > b.h_off_all.cap) throw std::runtime_error("internal: more input segments than the offset array was sized for");
    if (s.dst_r == 0) ho[0] = 0;  // (else the previous chunk wrote this entry; a lane may be reading it)
    // (on the packer's threads when it runs: a quarter of a million reads per chunk were 0.15 ms of the feeder's 0.56 per chunk)
    std::atomic<uint32_t> ml_all{0};
    std::atomic<bool> bad{false};
    auto narrow = [&](uint64_t i0, uint64_t i1) {
        const Narrowed nw = narrow_offsets(poff, i0, i1, s.dst_b, ho);
        if (nw.descending) bad.store(true);
        uint32_t cur = ml_all.load();
        while (nw.max_len > cur && !ml_all.compare_exchange_weak(cur, nw.max_len)) {}
    };
    if (packed && cnt >= (1u << 16)) pack_pool_for(cnt, 1u << 14, narrow);
    else narrow(0, cnt);
    if (bad.load()) throw std::runtime_error("arg: read_off is not ascending");
    // before anything is staged: the cut takes at least one read, so one long read makes nb larger than h_stage
    if (ml_all.load() > kMaxReadLen)
        throw std::runtime_error("limit: read of " + std::to_string(ml_all.load()) + " bases; this build verifies reads up to " + std::to_string(kMaxReadLen));
    return ml_all.load();
}

// chunk k: its offsets narrowed, its bases staged where they must be -- packed, or from ordinary memory: once the copy of
// chunk k - kStage has left the staging buffer --, the copies and the event issued, the chunk published
void Batch::HostRun::copy_chunk(size_t k, const FeedStep& s, uint8_t& prev_code) {
    const FeedView::Part& src_part = view.parts[s.part];
    const uint64_t* poff = src_part.off + s.part_read;  // this chunk's offsets inside its part
    Arena& ar = b.arena[s.seg & 1];
    uint32_t* ho = b.h_off_all.p + off_index(s.r, s.seg);
    const uint32_t ml = narrow_chunk(s, poff, ho);
    const double t0 = now_s();
    hipEvent_t ev = b.chunk_ev.at(k, hipEventDisableTiming);
    if (s.nb) {
        const uint8_t* src = src_part.bases + poff[0];
        if (packed || !src_part.pinned) {
            uint8_t* hs = b.h_stage[k % kStage].p;
            if (k >= kStage) {  // its last copy must have left (polled, like the watcher)
                for (;;) {
                    const hipError_t q = hipEventQuery(b.chunk_ev[k - kStage]);
                    if (q == hipSuccess) break;
                    if (q != hipErrorNotReady) throw_hip(q, "hipEventQuery(stage)", __FILE__, __LINE__);
                    std::this_thread::sleep_for(std::chrono::microseconds(20));
                }
            }
            if (packed) {
                if (s.dst_b == 0) prev_code = 0;  // a new segment
                prev_code = pack_chunk(hs, src, s.dst_b, s.nb, prev_code);
            } else {
                parallel_copy(hs, src, s.nb);
            }
            src = hs;
        }
        if (packed)
            HIP_CHECK(hipMemcpyAsync(ar.d_packed.p + (s.dst_b >> 1), src, ((s.dst_b + s.nb + 1) >> 1) - (s.dst_b >> 1), hipMemcpyHostToDevice, b.copy_stream));
        else
            HIP_CHECK(hipMemcpyAsync(ar.d_bases.p + s.dst_b, src, s.nb, hipMemcpyHostToDevice, b.copy_stream));
    }
    HIP_CHECK(hipMemcpyAsync(ar.d_off.p + s.dst_r, ho, (s.cnt() + 1) * 4, hipMemcpyHostToDevice, b.copy_stream));
    HIP_CHECK(hipEventRecord(ev, b.copy_stream));
    if (trace) fprintf(stderr, "[run_host] chunk %zu: reads %llu..%llu (%.1f MB, segment %llu) issued at %.2f ms (host side %.2f ms)\n", k, (unsigned long long)s.r, (unsigned long long)s.e, s.nb / 1e6, (unsigned long long)s.seg, (now_s() - b.run_t0) * 1e3, (now_s() - t0) * 1e3);
    {
        std::lock_guard<std::mutex> lk(mu);
        chunks.push_back(Chunk{s.r, s.e, ml, (uint32_t)s.seg, ev});
        if (s.e == n) issued_all = true;
    }
    cv.notify_all();
}

// Only the WATCHER thread looks at the copies' events, by polling, and publishes what has arrived (lanes that blocked in
// hipEventSynchronize while a third lane sat in hipStreamSynchronize kept that lane from returning for 10 ms at a time).
void Batch::HostRun::watch() {
    try {
        HIP_CHECK(hipSetDevice(b.di->device));
        size_t c = 0;
        for (;;) {
            size_t upto;
            bool last;
            std::vector<hipEvent_t> evs;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (abort) return;
                upto = chunks.size();
                last = issued_all;
                for (size_t i = c; i < upto; i++) evs.push_back(chunks[i].ev);
            }
            const size_t c0 = c;
            while (c < upto) {
                const hipError_t q = hipEventQuery(evs[c - c0]);
                if (q == hipSuccess) c++;
                else if (q == hipErrorNotReady) break;
                else throw_hip(q, "hipEventQuery(chunk)", __FILE__, __LINE__);
            }
            if (c != c0) {
                {
                    std::lock_guard<std::mutex> lk(mu);
                    n_complete = c;
                }
                cv.notify_all();
            }
            if (last && c == upto) return;
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    } catch (...) {
        fail(std::current_exception());
    }
}

// ---- lanes ----
void Batch::HostRun::lane_loop(Batch* lane) {
    try {
        HIP_CHECK(hipSetDevice(b.di->device));
        uint64_t last_done = ~0ull;  // the last range this lane finished
        for (;;) {
            Taken t;
            if (!take_range(lane, last_done, t)) return;
            cv.notify_all();
            run_range_on_lane(lane, t);
            finish_range(lane, t);
            last_done = t.k;
            cv.notify_all();
        }
    } catch (...) {
        fail(std::current_exception());
    }
}

// waits until range_take gives the lane a range; false: failed elsewhere, or every read taken
bool Batch::HostRun::take_range(Batch* lane, uint64_t last_done, Taken& t) {
    std::unique_lock<std::mutex> lk(mu);
    // The lane's result array only has to hold hits until they have left for the host: once it is half full and everything
    // in it has been committed, start again at its beginning (a 100 M-read host batch would otherwise pile a third of its
    // hits up on the device).
    if (!b.keep_on_device && lane->n_hits_total > lane->d_hits.cap / 2 && (last_done == ~0ull || last_done < next_commit)) {
        HIP_CHECK(hipStreamSynchronize(b.copy_stream2));
        lane->n_hits_total = 0;
    }
    for (;;) {
        if (abort || next_read >= n) return false;
        const uint64_t arrived = n_complete ? chunks[n_complete - 1].end : 0;
        const bool all_arrived = issued_all && n_complete == chunks.size();
        const RangeRoom room = range_room(seg_begin, n, next_read, arrived);  // a range stays inside one segment
        const uint64_t take = range_take(n, next_read, b.ws_reads, ramp_floor, idle_take, n_lanes_used, room.avail, all_arrived || room.closed, busy_lanes);
        if (take) {
            t.rb = next_read;
            t.re = next_read + take;
            next_read = t.re;
            t.seg = (uint32_t)room.seg;
            t.seg_first = room.seg_first;
            for (size_t c = 0; c < n_complete; c++)  // (a few dozen chunks)
                if (chunks[c].end > t.rb && chunks[c].begin < t.re) t.ml = std::max(t.ml, chunks[c].max_len);
            t.k = ranges.size();
            ranges.emplace_back();
            ranges[t.k].begin = t.rb, ranges[t.k].end = t.re;
            busy_lanes++;
            return true;
        }
        cv.wait(lk);  // for the next copy to arrive (the watcher publishes them), or for a lane to finish (the idle rule)
    }
}

void Batch::HostRun::run_range_on_lane(Batch* lane, Taken& t) {
    const Arena& ar = b.arena[t.seg & 1];
    const uint32_t* ho = b.h_off_all.p + off_index(t.rb, t.seg);  // offsets of reads rb .. re inside segment seg
    const uint32_t* dso = ar.d_off.p + (t.rb - t.seg_first);
    t.hit_off = lane->n_hits_total;
    t.a_off = lane->n_assign_total;
    const double t0 = now_s();
    // base normalisation (binner.rs:88-100) in place, on the lane's own stream: a kernel on the copy stream would queue
    // behind the persistent verification kernels of the other lanes
    if (packed) launch_unpack(lane->stream, ar.d_packed.p, ar.d_bases.p, ho[0], ho[t.re - t.rb]);
    else launch_normalise(lane->stream, ar.d_bases.p, ar.d_bases.p, ho[0], ho[t.re - t.rb]);
    lane->run_slice(p, ar.d_bases.p, dso, ho, t.re - t.rb, t.ml, read_base + t.rb);
    if (trace) fprintf(stderr, "[run_host] range %llu (reads %llu..%llu): kernels %.1f ms, done at %.1f ms\n", (unsigned long long)t.k, (unsigned long long)t.rb, (unsigned long long)t.re, (now_s() - t0) * 1e3, (now_s() - b.run_t0) * 1e3);
}

void Batch::HostRun::finish_range(Batch* lane, const Taken& t) {
    std::lock_guard<std::mutex> lk(mu);
    Range& rg = ranges[t.k];
    rg.lane = lane;
    rg.hit_off = t.hit_off;
    rg.hit_cnt = lane->n_hits_total - t.hit_off;
    rg.a_off = t.a_off;
    rg.a_cnt = lane->n_assign_total - t.a_off;
    rg.done = true;
    b.max_len = std::max(b.max_len, t.ml);
    busy_lanes--;
    commit_ready();
}

// mu held: hits and assignments of finished ranges leave for the host in read order
void Batch::HostRun::commit_ready() {
    while (next_commit < ranges.size() && ranges[next_commit].done) {
        Range& rg = ranges[next_commit];
        if (rg.hit_cnt && stage_hits) {
            PinnedStage& st = b.hits_stage;
            st.reserve(st.staged + rg.hit_cnt, b.copy_stream2);
            HIP_CHECK(hipMemcpyAsync(st.at(st.staged), rg.lane->d_hits.p + rg.hit_off, rg.hit_cnt * sizeof(mtsv_hit), hipMemcpyDeviceToHost, b.copy_stream2));
            st.staged += rg.hit_cnt;
        }
        if (rg.a_cnt && stage_assign) {
            PinnedStage& st = b.assign_stage;
            st.reserve(st.staged + rg.a_cnt, b.copy_stream2);
            HIP_CHECK(hipMemcpyAsync(st.at(st.staged), rg.lane->d_assign.p + rg.a_off * a_rec, rg.a_cnt * a_rec, hipMemcpyDeviceToHost, b.copy_stream2));
            st.staged += rg.a_cnt;
        }
        b.segments.push_back(Segment{rg.lane, rg.hit_off, rg.hit_cnt, 0, 0, rg.a_off, rg.a_cnt});
        done_prefix = rg.end;
        next_commit++;
    }
}

// The feeder, the watcher and a thread per further lane; the caller's thread is lane 0.  On every way out the threads are
// joined, then commit_mu is cleared.  A thread that cannot be created fails the run: those that run see abort and return.
void Batch::HostRun::run_threads() {
    CommitMutexScope commit(b.commit_mu, mu);
    JoinedThreads th;
    try {
        th.th.emplace_back([this] { feed(); });
        th.th.emplace_back([this] { watch(); });
        for (uint64_t i = 1; i < n_lanes_used; i++) th.th.emplace_back([this, lane = lanes[i]] { lane_loop(lane); });
    } catch (...) {
        fail(std::current_exception());
        return;
    }
    lane_loop(&b);
}

// the first error rethrown; else end_run, the last copies waited for, and what the run staged checked against its totals
void Batch::HostRun::finish() {
    if (trace) fprintf(stderr, "[run_host] threads joined at %.1f ms\n", (now_s() - b.run_t0) * 1e3);
    if (first_err) {
        (void)hipStreamSynchronize(b.copy_stream);
        (void)hipStreamSynchronize(b.copy_stream2);
        std::rethrow_exception(first_err);
    }
    b.end_run();
    HIP_CHECK(hipStreamSynchronize(b.copy_stream2));
    PinnedStage &hs = b.hits_stage, &as = b.assign_stage;
    hs.valid = stage_hits && hs.staged == b.total_hits;
    b.host_hits_dropped = !stage_hits && !b.keep_on_device;
    if (stage_assign) {
        uint64_t total_a = 0;
        for (auto& sg : b.segments) total_a += sg.a_count;
        as.valid = as.staged == total_a;
        if (!as.valid) throw std::runtime_error("internal: run_host staged " + std::to_string(as.staged) + " of " + std::to_string(total_a) + " assignments");
    }
    b.last_run = seg_begin.size() == 1 ? kRunHostOneSegment : kRunHostSegments;
    if (trace) fprintf(stderr, "[run_host] hits on the host at %.1f ms (%llu ranges, %llu chunks); %.1f ms since the call began\n", (now_s() - b.run_t0) * 1e3, (unsigned long long)ranges.size(), (unsigned long long)chunks.size(), (now_s() - t_entry) * 1e3);
    if (!hs.valid && stage_hits) throw std::runtime_error("internal: run_host staged " + std::to_string(hs.staged) + " of " + std::to_string(b.total_hits) + " hits");
}

// The same for a batch that lies in several pieces (mtsv_batch_run_host_parts: a host that parses its input in blocks hands
// several blocks to one call -- larger passes on the device -- without putting them together first).  The reads are
// numbered through the parts in order.
void Batch::run_host_parts(const HostPart* parts, int n_parts, const mtsv_params& p, uint64_t read_base) {
    HostRun run(*this, parts, n_parts, p, read_base);
    run.begin();
    run.run_threads();
    run.finish();
}

}  // namespace mtsv
