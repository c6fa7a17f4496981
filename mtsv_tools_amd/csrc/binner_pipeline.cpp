// binner_pipeline.cpp -- the pipelined run of mtsv-binner: every mode but --fold-on-gpu.  Overlapped stages (the reference
// overlaps producer / workers / joiner the same way, vendor/cue/src/lib.rs:45-105): the producer parses FASTX into numbered
// batches, GPU workers (several per --devices entry; two dispatchers over all chunks in chunk mode) take batches as they
// come, a writer thread formats and writes the result lines in input order.
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <thread>

#include "binner_run.hpp"

namespace mtsv_cli {
namespace {

struct Work {
    std::unique_ptr<ReadBlock> rb;
    uint64_t seq = 0;
    mtsv_hit* hits = nullptr;  // this batch's hits: a slice of the array hits_owner holds (read numbers: the call's, read_first + the batch's)
    uint64_t n_hits = 0;
    uint64_t read_first = 0;  // the batch's first read in the numbering of its call (the formatter subtracts it)
    std::shared_ptr<void> hits_owner;  // the result array of the library call the batch was part of
    // MTSV_CLI_ASSIGN=1, MTSV_CLI_ASSIGN_LONG=1: the batch's assignments instead (the same slicing and numbering; records of
    // a_rec bytes that begin with the read), and their array
    uint8_t* assigns = nullptr;
    uint64_t n_assigns = 0;
    std::shared_ptr<void> assigns_owner;
    std::shared_ptr<uint64_t> flags;   // --matched / --unmatched: the match flags of that call; read i of the batch is bit read_first + i
};
using Group = std::vector<std::unique_ptr<Work>>;

class Queue {
   public:
    size_t cap = 2;
    size_t n_takers = 1;  // threads that call pop_group
    void push(std::unique_ptr<Work> w) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return q_.size() < cap || closed_; });
        q_.push_back(std::move(w));
        cv_.notify_all();
    }
    // the next batches in order, up to max_reads reads / max_n batches: a full group, or -- when the input has ended or
    // `idle` says that the device has nothing else to do -- whatever is waiting
    // (max_bases: a group holds at most that many bases -- or one batch)
    Group pop_group(uint64_t max_reads, size_t max_n, const std::function<bool()>& idle, uint64_t max_bases) {
        std::unique_lock<std::mutex> lk(mu_);
        auto waiting = [&] {
            uint64_t r = 0;
            for (auto& w : q_) r += w->rb->n();
            return r;
        };
        for (;;) {
            if (!q_.empty() && (closed_ || q_.size() >= max_n || waiting() >= max_reads || idle())) break;
            if (q_.empty() && closed_) return {};
            cv_.wait_for(lk, std::chrono::microseconds(200));  // (idle() changes without a notification)
        }
        // (the input has ended: what is left is shared out, so that the workers finish together)
        if (closed_ && n_takers > 1) max_n = std::min(max_n, (q_.size() + n_takers - 1) / n_takers);
        Group g;
        uint64_t r = 0, nb = 0;
        while (!q_.empty() && g.size() < max_n && r < max_reads) {
            nb += q_.front()->rb->bases.size();
            if (!g.empty() && nb > max_bases) break;
            r += q_.front()->rb->n();
            g.push_back(std::move(q_.front()));
            q_.pop_front();
        }
        cv_.notify_all();
        return g;
    }
    std::unique_ptr<Work> pop() {  // nullptr: closed and empty
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return nullptr;
        auto w = std::move(q_.front());
        q_.pop_front();
        cv_.notify_all();
        return w;
    }
    void close() {
        std::lock_guard<std::mutex> lk(mu_);
        closed_ = true;
        cv_.notify_all();
    }

   private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::unique_ptr<Work>> q_;
    bool closed_ = false;
};

// helper threads of the result side: the formatting of a batch's hits runs on them in parallel, and the
// finished text of batch k is written (positional writes at offsets fixed in batch order) while batch k+1
// is being formatted
class Helpers {
   public:
    explicit Helpers(unsigned n) {
        for (unsigned i = 0; i < n; i++) th_.emplace_back([this] { serve(); });
    }
    void submit(std::function<void()> f) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_.push_back(std::move(f));
        }
        cv_.notify_one();
    }
    void wait_all() { wait_below(1); }
    void wait_below(size_t n) {  // until fewer than n jobs are queued or running
        std::unique_lock<std::mutex> lk(mu_);
        idle_.wait(lk, [&] { return q_.size() + running_ < n; });
    }
    // f(0) .. f(parts - 1), the first on this thread and the others on the helpers; returns when all have
    template <class F>
    void run_parts(unsigned parts, const F& f) {
        for (unsigned k = 1; k < parts; k++) submit([&f, k] { f(k); });
        f(0);
        if (parts > 1) wait_all();
    }
    ~Helpers() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }

   private:
    void serve() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                f = std::move(q_.front());
                q_.pop_front();
                running_++;
            }
            f();
            {
                std::lock_guard<std::mutex> lk(mu_);
                running_--;
            }
            idle_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, idle_;
    std::deque<std::function<void()>> q_;
    std::vector<std::thread> th_;
    size_t running_ = 0;
    bool stop_ = false;
};

struct JoinOnExit {  // (an early return must not leave the thread running)
    std::thread& t;
    ~JoinOnExit() {
        if (t.joinable()) t.join();
    }
};
struct InFlight {  // a library call of some worker is running
    std::atomic<int>& c;
    explicit InFlight(std::atomic<int>& n) : c(n) { c++; }
    ~InFlight() { c--; }
};

// MTSV_CLI_TIMING=1: where the stages of the command line spend their time (microseconds, summed per stage)
struct StageTimes {
    std::atomic<uint64_t> ingest_wait{0}, push_wait{0}, gpu{0}, gpu_wait{0}, fmt{0}, done_wait{0}, write_wait{0};
    static void add(std::atomic<uint64_t>& a, double s) { a.fetch_add((uint64_t)(s * 1e6)); }
};

// what one library call on a group of batches brought down
struct CallResult {
    mtsv_hit* hits = nullptr;
    uint64_t n_hits = 0;
    uint8_t* assigns = nullptr;  // records of a_rec bytes
    uint64_t n_assigns = 0;
    std::shared_ptr<uint64_t> flags;
};

int env_int(const char* name, int otherwise) {
    const char* e = getenv(name);
    return e ? atoi(e) : otherwise;
}

class PipelinedRun {
   public:
    PipelinedRun(const Run& run, Producer& producer, Outputs& outputs);
    int run();

   private:
    bool load_indexes();
    bool make_workspaces();
    int make_ws(size_t wk);
    int set_switches(mtsv_batch* ws) const;
    void read_input();
    void write_output(Helpers& fmt_pool, Helpers& write_pool);
    void write_sides(Work& w, Helpers& fmt_pool, Helpers& write_pool);
    bool format_and_write(Work& w, Helpers& fmt_pool, Helpers& write_pool);
    void write_at(Helpers& write_pool, int fd, std::shared_ptr<void> owner, const char* data, uint64_t len, off_t at);
    void gpu_worker(size_t wk);
    void run_group(size_t wk, Group& group);
    int call_merged(size_t wk, Work& w, CallResult& r);
    int call_parts(size_t wk, Group& group, uint64_t group_reads, CallResult& r);
    int download_records(mtsv_batch* from, CallResult& r) const;
    void hand_out(Group& group, const CallResult& r);
    bool gather_taxa(TaxaSum& sum);
    void print_timing() const;
    void mark(const std::string& what);
    uint64_t& record_read(uint8_t* records, uint64_t i) const { return *reinterpret_cast<uint64_t*>(records + i * a_rec_); }

    const Run& run_;
    Producer& producer_;
    Outputs& out_;
    const mtsv_params& p_;
    const unsigned host_threads_;
    const bool chunked_, merged_, filtered_, partition_;
    const size_t n_filters_;
    // what the run is sized by (the constructor says how)
    int match_mode_;
    bool cli_assign_long_, cli_records_;
    uint64_t a_rec_;
    uint64_t group_reads_;  // reads of one library call, MTSV_CLI_GROUP_READS
    size_t group_max_, workers_per_device_, n_workers_;
    bool small_input_;
    uint32_t warm_len_;
    uint64_t merge_reads_, merge_bases_, chain_reads_, chain_bases_;
    const bool cli_timing_ = getenv("MTSV_CLI_TIMING") != nullptr;
    // the library's objects: the database's index (or chunks) and the filter indexes, and per worker its workspace
    // (--merge-on-gpu: its collector), its filter stages' and (--merge-on-gpu) its chunks'
    std::vector<IndexPtr> idx_, fidx_;
    std::vector<int> chunk_dev_;
    std::vector<BatchPtr> ws_;
    std::vector<std::vector<BatchPtr>> fws_, cws_;
    // the run
    Queue parsed_, done_;
    ExitCode code_;
    std::atomic<bool> write_failed_{false};
    std::atomic<int> calls_in_flight_{0};
    std::atomic<uint64_t> reads_matched_{0}, reads_partitioned_{0};
    std::vector<std::atomic<uint64_t>> stage_in_, stage_removed_;  // --filter-index: reads into / dropped by each stage
    uint64_t n_batches_ = 0;
    StageTimes t_;
    double t_begin_ = 0;
    std::mutex marks_mu_;
    std::vector<std::pair<std::string, double>> marks_;  // (what, seconds since the queries began), printed with the timing
};

PipelinedRun::PipelinedRun(const Run& run, Producer& producer, Outputs& outputs)
    : run_(run), producer_(producer), out_(outputs), p_(run.params), host_threads_(run.host_threads), chunked_(run.chunked()), merged_(run.merged()),
      filtered_(run.filtered), partition_(run.partition), n_filters_(run.filter_paths.size()), stage_in_(n_filters_), stage_removed_(n_filters_) {
    for (size_t k = 0; k < n_filters_; k++) stage_in_[k] = 0, stage_removed_[k] = 0;
    // (--merge-on-gpu: the flags come from the merged hits, so the hits are gathered with or without a results file)
    match_mode_ = !partition_ ? MTSV_MATCH_OFF : (run.have_results() || merged_) ? MTSV_MATCH_WITH_HITS : MTSV_MATCH_ONLY;
    // MTSV_CLI_ASSIGN=1: the default results format is written from assignments -- the smallest edit per read and TaxID,
    // reduced on the device (mtsv_batch_set_assignments, MTSV_ASSIGN_ONLY: no hit crosses to the host) -- where one workspace
    // per worker holds a call's hits: a single index (behind --filter-index: the database's workspace) or the collector of
    // --merge-on-gpu.  The file is the same byte for byte.  --output-format long stays on the hits under this switch.
    // The default is 0 (profiles/README.md r14: the measurement and what it decided).
    // MTSV_CLI_ASSIGN_LONG=1: the same for --output-format long -- the workspace in MTSV_GRAIN_LONG, one 24-byte record per read
    // and (TaxID, GI, offset) with the smallest edit, the file written by mtsv_format_assignments_gi, byte for byte the same.
    // A switch of its own: MTSV_CLI_ASSIGN alone leaves long output on the hits.  Default 0, not measured yet.
    const bool from_records = run.have_results() && (!chunked_ || merged_) && match_mode_ != MTSV_MATCH_ONLY;
    const bool cli_assign = env_int("MTSV_CLI_ASSIGN", 0) != 0 && from_records && !run.long_fmt;
    cli_assign_long_ = env_int("MTSV_CLI_ASSIGN_LONG", 0) != 0 && from_records && run.long_fmt;
    cli_records_ = cli_assign || cli_assign_long_;  // the results file is written from assignment records
    a_rec_ = cli_assign_long_ ? sizeof(mtsv_assignment_gi) : sizeof(mtsv_assignment);
    // (both record types begin with the 8-byte read: record_read() relies on it)
    static_assert(offsetof(mtsv_assignment, read) == 0 && offsetof(mtsv_assignment_gi, read) == 0, "records begin with the read");
    // One library call takes every batch that is waiting, up to group_reads_ reads (mtsv_batch_run_host_parts): the device
    // is several times faster on passes of a million reads than on a quarter of that (a pass costs ~2.5 ms before it does
    // any work), while the parser is fastest on blocks of ~80 MB.
    group_reads_ = std::max<uint64_t>(run.batch_reads, 1ull << 20);
    if (const char* e = getenv("MTSV_CLI_GROUP_READS")) group_reads_ = std::max<uint64_t>(run.batch_reads, strtoull(e, nullptr, 10));
    group_max_ = (size_t)std::min<uint64_t>(32, std::max<uint64_t>(1, group_reads_ / std::max<uint64_t>(run.batch_reads, 1)));
    // Several workers per --devices entry, a workspace of ONE lane each: a call is copy in -> kernels -> hits out, and
    // what overlaps on the device are the calls of different workers (tools/call_stream.py: one worker with the
    // default three lanes 165 M reads/s on megaread calls, three workers of one lane 229 M).
    // (three workers on groups of 1 Mi reads: 0.210 s for 32 M reads twice over; two on 512 Ki: 0.225-0.245 -- since the
    //  parser stopped copying its blocks the workers are what a run waits for)
    workers_per_device_ = (size_t)std::max(1, std::min(8, env_int("MTSV_CLI_WORKERS", 3)));
    // (a small input is through before the extra workspaces have paid for themselves)
    uint64_t input_bytes = 0;
    struct stat st;
    if (stat(run.input.c_str(), &st) == 0) input_bytes = (uint64_t)st.st_size;
    small_input_ = input_bytes < (256ull << 20) && !getenv("MTSV_CLI_WORKERS");
    if (small_input_) workers_per_device_ = 1;
    n_workers_ = chunked_ && !merged_ ? 2 : run.devices.size() * workers_per_device_;
    warm_len_ = producer.warm_len();
    // --merge-on-gpu: a call is one block of reads, resident in a workspace per chunk
    merge_reads_ = block_reads_max(run.batch_reads);
    merge_bases_ = workspace_bases(merge_reads_, warm_len_, 1 << 22);
    // --filter-index: the later stages and the database's workspace receive a call's reads in HBM and hold them as one
    // resident batch: room for the bases of a call (a call whose blocks hold more is cut into several)
    chain_reads_ = call_reads_max(group_reads_, run.batch_reads);
    chain_bases_ = workspace_bases(chain_reads_, warm_len_, 0);
    parsed_.cap = (n_workers_ + 1) * group_max_ + 1;
    parsed_.n_takers = n_workers_;
    done_.cap = n_workers_ * group_max_ + 1;
}

void PipelinedRun::mark(const std::string& what) {
    if (!cli_timing_) return;
    std::lock_guard<std::mutex> lk(marks_mu_);
    marks_.emplace_back(what, now_s() - t_begin_);
}

bool PipelinedRun::load_indexes() {
    const std::vector<int>& devices = run_.devices;
    idx_.resize(run_.index_paths.size());
    chunk_dev_.resize(idx_.size());
    for (size_t c = 0; c < idx_.size(); c++) {
        chunk_dev_[c] = devices[c % devices.size()];
        if (mtsv_index_load(run_.index_paths[c].c_str(), out(idx_[c])) != MTSV_OK) return code_.lib_error();
        // one index: resident on every listed device; chunks: chunk c on its device
        for (size_t d = 0; d < (chunked_ ? 1 : devices.size()); d++)
            if (mtsv_index_to_device(idx_[c].get(), chunked_ ? chunk_dev_[c] : devices[d], MTSV_DEV_DEFAULT) != MTSV_OK) return code_.lib_error();
    }
    // the filter indexes: every one resident on every listed device, beside the database
    fidx_.resize(n_filters_);
    for (size_t c = 0; c < n_filters_; c++) {
        if (mtsv_index_load(run_.filter_paths[c].c_str(), out(fidx_[c])) != MTSV_OK) return code_.lib_error();
        for (size_t d = 0; d < devices.size(); d++)
            if (mtsv_index_to_device(fidx_[c].get(), devices[d], MTSV_DEV_DEFAULT) != MTSV_OK) return code_.lib_error();
    }
    return true;
}

// the switches of a worker's main workspace (after the warm-up reads, which are not the run's)
int PipelinedRun::set_switches(mtsv_batch* ws) const {
    int rc = MTSV_OK;
    if (run_.have_report()) rc = mtsv_batch_set_taxa_report(ws, 1);
    if (rc == MTSV_OK && partition_) rc = mtsv_batch_set_match_flags(ws, match_mode_);
    if (rc == MTSV_OK && cli_assign_long_) rc = mtsv_batch_set_assignment_grain(ws, MTSV_GRAIN_LONG);
    if (rc == MTSV_OK && cli_records_) rc = mtsv_batch_set_assignments(ws, MTSV_ASSIGN_ONLY);
    return rc;
}

// worker wk's workspaces: created, sized for the calls to come and run once on reads sampled from the index
// (mtsv_batch_reserve_host)
int PipelinedRun::make_ws(size_t wk) {
    const uint64_t call_reads = chain_reads_;
    const int dev = run_.devices[wk % run_.devices.size()];
    const bool warm = !small_input_ && !getenv("MTSV_CLI_COLD");
    auto warm_up = [&](mtsv_batch* ws, uint64_t reads) { return mtsv_batch_reserve_host(ws, reads, reads * (uint64_t)(warm_len_ + warm_len_ / 8), warm_len_); };
    if (merged_) {
        int rc = mtsv_batch_create_lanes(idx_[0].get(), dev, 1024, 1 << 16, 0, 1, out(ws_[wk]));
        for (size_t c = 0; c < idx_.size() && rc == MTSV_OK; c++) {
            rc = mtsv_batch_create_lanes(idx_[c].get(), dev, merge_reads_, merge_bases_, 0, 1, out(cws_[wk][c]));
            if (rc == MTSV_OK && warm) rc = warm_up(cws_[wk][c].get(), 4096);
        }
        return rc == MTSV_OK ? set_switches(ws_[wk].get()) : rc;
    }
    // (a workspace that receives its reads from a filter stage runs them as one resident batch: room for all of them)
    auto create = [&](mtsv_index* ix, bool resident, BatchPtr& ws) {
        const uint64_t ws_bases = resident ? chain_bases_ : 1 << 22;
        return workers_per_device_ > 1 ? mtsv_batch_create_lanes(ix, dev, call_reads, ws_bases, 0, 1, out(ws))
                                       : mtsv_batch_create(ix, dev, resident ? call_reads : mtsv_bin_batch_workspace_reads(call_reads), ws_bases, 0, out(ws));
    };
    int rc = create(idx_[0].get(), filtered_, ws_[wk]);
    // (only the workspace that takes the host batches needs their arenas; the others are warmed on a small batch)
    if (rc == MTSV_OK && warm) rc = warm_up(ws_[wk].get(), filtered_ ? 4096 : call_reads);
    for (size_t k = 0; k < n_filters_ && rc == MTSV_OK; k++) {
        rc = create(fidx_[k].get(), k > 0, fws_[wk][k]);
        if (rc == MTSV_OK && warm) rc = warm_up(fws_[wk][k].get(), k ? 4096 : call_reads);
        if (rc == MTSV_OK) rc = mtsv_batch_set_match_flags(fws_[wk][k].get(), MTSV_MATCH_ONLY);  // (after the warm-up reads)
    }
    return rc == MTSV_OK ? set_switches(ws_[wk].get()) : rc;
}

// the workers' workspaces: part of the device set-up, like making the index resident; every worker's on a thread of its own
bool PipelinedRun::make_workspaces() {
    const size_t n = chunked_ && !merged_ ? 0 : n_workers_;  // (chunk mode: mtsv_bin_batch_chunks brings its own)
    ws_.resize(n);
    fws_.resize(n);
    for (auto& stages : fws_) stages.resize(n_filters_);
    cws_.resize(merged_ ? n : 0);
    for (auto& chunks : cws_) chunks.resize(idx_.size());
    std::vector<int> rc(n, MTSV_OK);
    std::vector<std::string> msg(n);
    auto make = [&](size_t wk) {
        rc[wk] = make_ws(wk);
        if (rc[wk] != MTSV_OK) msg[wk] = mtsv_last_error();  // (thread-local)
    };
    std::vector<std::thread> th;
    for (size_t wk = 1; wk < n; wk++) th.emplace_back(make, wk);
    if (n) make(0);
    for (auto& t : th) t.join();
    for (size_t wk = 0; wk < n; wk++)
        if (rc[wk] != MTSV_OK) return code_.lib_error(msg[wk]);
    return true;
}

void PipelinedRun::read_input() {
    double t_last = now_s();
    const bool ok = producer_.produce(run_.batch_reads, [&](std::unique_ptr<ReadBlock> rb) {
        if (code_.failed()) return false;
        auto w = std::make_unique<Work>();
        w->rb = std::move(rb);
        w->seq = n_batches_++;
        const double t_a = now_s();
        if (w->seq == 0) mark("first block parsed");
        StageTimes::add(t_.ingest_wait, t_a - t_last);  // producing this batch (mostly: waiting for the parser threads)
        parsed_.push(std::move(w));
        t_last = now_s();
        StageTimes::add(t_.push_wait, t_last - t_a);  // waiting for room in the queue to the GPU workers
        return true;
    });
    if (!ok) {
        logmsg("ERROR", "Unable to read from input file: " + producer_.error());
        code_.set(12);  // binner.rs:81-84
    }
    parsed_.close();
    mark("reader done");
}

// a positional write on the write pool; `owner` keeps the bytes until it is done
void PipelinedRun::write_at(Helpers& write_pool, int fd, std::shared_ptr<void> owner, const char* data, uint64_t len, off_t at) {
    write_pool.submit([this, fd, owner, data, len, at] {
        if (pwrite_all(fd, data, len, at)) return;
        write_failed_.store(true);
        code_.set(11);  // binner.rs:136-139: the producer and the workers stop at once
    });
}

// --matched / --unmatched: the batch's records, each to its side, serialised over ranges of reads in parallel and
// written at offsets fixed in batch order, like the result lines
void PipelinedRun::write_sides(Work& w, Helpers& fmt_pool, Helpers& write_pool) {
    const uint64_t n_reads = w.rb->n();
    const unsigned pp = n_reads >= (1u << 14) ? host_threads_ : 1;
    std::vector<std::string> side[2];
    side[0].resize(pp);
    side[1].resize(pp);
    const ReadBlock& blk = *w.rb;
    const uint64_t* fw = w.flags.get();
    const uint64_t first = w.read_first;
    const bool fastq = run_.fastq;
    const bool want[2] = {out_.part_fd[0] >= 0, out_.part_fd[1] >= 0};
    fmt_pool.run_parts(pp, [&](unsigned k) {
        const uint64_t r0 = n_reads * k / pp, r1 = n_reads * (k + 1) / pp;
        for (int sd = 0; sd < 2; sd++)
            if (want[sd]) side[sd][k].reserve((size_t)((blk.off[r1] - blk.off[r0]) * (fastq ? 2 : 1) + (r1 - r0) * 48));
        for (uint64_t i = r0; i < r1; i++) {
            const uint64_t bit = first + i;
            const int sd = (fw[bit >> 6] >> (bit & 63)) & 1 ? 0 : 1;
            if (want[sd]) mtsv_ingest::write_block_record(side[sd][k], fastq, blk, i);
        }
    });
    for (int sd = 0; sd < 2; sd++)
        for (unsigned k = 0; k < pp && want[sd]; k++) {
            if (side[sd][k].empty()) continue;
            auto tx = std::make_shared<std::string>(std::move(side[sd][k]));
            write_at(write_pool, out_.part_fd[sd], tx, tx->data(), tx->size(), out_.part_pos[sd]);
            out_.part_pos[sd] += (off_t)tx->size();
        }
    reads_partitioned_ += n_reads;
}

// write_assignments over slices of the batch's hits (cut between reads), one thread each; the text to the write pool.
// False: a library error (logged), nothing written.
bool PipelinedRun::format_and_write(Work& w, Helpers& fmt_pool, Helpers& write_pool) {
    const uint64_t n_reads = w.rb->n();
    const uint64_t n_items = cli_records_ ? w.n_assigns : w.n_hits;
    auto read_of = [&](uint64_t i) { return cli_records_ ? record_read(w.assigns, i) : w.hits[i].read; };
    const unsigned parts = n_items >= (1u << 16) ? host_threads_ : 1;
    std::vector<uint64_t> cut(parts + 1, n_items);
    cut[0] = 0;
    for (unsigned k = 1; k < parts; k++) {
        uint64_t c = std::max(cut[k - 1], n_items * k / parts);
        while (c > cut[k - 1] && c < n_items && read_of(c) == read_of(c - 1)) c++;
        cut[k] = c;
    }
    std::vector<ArrayPtr<char>> text(parts);
    std::vector<uint64_t> len(parts, 0);
    std::vector<int> rc(parts, MTSV_OK);
    std::vector<std::string> msg(parts);
    const char* ids = w.rb->ids.data();
    const uint64_t* id_off = w.rb->id_off.data();
    fmt_pool.run_parts(parts, [&](unsigned k) {
        if (out_.out_fd < 0) return;  // (no results file: --matched / --unmatched alone)
        const uint64_t n = cut[k + 1] - cut[k];
        if (cli_records_) {
            if (w.read_first)
                for (uint64_t i = cut[k]; i < cut[k + 1]; i++) record_read(w.assigns, i) -= w.read_first;
            const uint8_t* recs = w.assigns + cut[k] * a_rec_;
            rc[k] = cli_assign_long_ ? mtsv_format_assignments_gi((const mtsv_assignment_gi*)recs, n, ids, id_off, n_reads, out(text[k]), &len[k])
                                     : mtsv_format_assignments((const mtsv_assignment*)recs, n, ids, id_off, n_reads, out(text[k]), &len[k]);
        } else {
            if (w.read_first)
                for (uint64_t i = cut[k]; i < cut[k + 1]; i++) w.hits[i].read -= w.read_first;
            rc[k] = mtsv_format_results(w.hits + cut[k], n, ids, id_off, n_reads, run_.long_fmt, out(text[k]), &len[k]);
        }
        if (rc[k] != MTSV_OK) msg[k] = mtsv_last_error();  // thread-local
    });
    w.hits_owner.reset();  // (the array goes back to the library's pool with the last batch of its call)
    w.assigns_owner.reset();
    for (unsigned k = 0; k < parts; k++)
        if (rc[k] != MTSV_OK) return code_.lib_error(msg[k]);
    if (code_.failed() || write_failed_.load() || out_.out_fd < 0) return true;
    for (unsigned k = 0; k < parts; k++) {
        std::shared_ptr<char> tx(text[k].release(), ArrayFree{});  // the write job owns it now
        write_at(write_pool, out_.out_fd, tx, tx.get(), len[k], out_.out_pos);
        out_.out_pos += (off_t)len[k];
    }
    return true;
}

// the writer thread: the finished batches in input order
void PipelinedRun::write_output(Helpers& fmt_pool, Helpers& write_pool) {
    uint64_t total = 0, next_seq = 0;
    Group held;  // batches that finished ahead of their turn
    for (;;) {
        std::unique_ptr<Work> w;
        for (auto& h : held)
            if (h && h->seq == next_seq) {
                w = std::move(h);
                h = std::move(held.back());
                held.pop_back();
                break;
            }
        if (!w) {
            const double t_a = now_s();
            w = done_.pop();
            StageTimes::add(t_.done_wait, now_s() - t_a);
            if (!w) break;
            if (w->seq != next_seq) {
                held.push_back(std::move(w));
                continue;
            }
        }
        next_seq++;
        const double t_f0 = now_s();
        const uint64_t n_reads = w->rb->n();
        if (partition_ && w->flags && !code_.failed() && !write_failed_.load()) write_sides(*w, fmt_pool, write_pool);
        w->flags.reset();
        const bool ok = format_and_write(*w, fmt_pool, write_pool);
        // at most about two batches of text wait for the disk: the file stays a prefix of the results up to the
        // writes in flight (resume reads its last line), and formatted text does not pile up behind a slow disk
        const double t_a = now_s();
        StageTimes::add(t_.fmt, t_a - t_f0);
        write_pool.wait_below(2 * (size_t)host_threads_ + 1);
        StageTimes::add(t_.write_wait, now_s() - t_a);
        producer_.pool.put(std::move(w->rb));
        if (!ok) continue;
        total += n_reads;
        logmsg("DEBUG", "taxonomic binning: " + std::to_string(total) + " reads done");
    }
    write_pool.wait_all();
    if (write_failed_.load()) {
        logmsg("ERROR", "Error writing to result file");
        code_.set(11);  // binner.rs:136-139
    }
}

int PipelinedRun::download_records(mtsv_batch* from, CallResult& r) const {
    return cli_assign_long_ ? mtsv_batch_download_assignments_gi(from, (mtsv_assignment_gi**)&r.assigns, &r.n_assigns, nullptr)
                            : mtsv_batch_download_assignments(from, (mtsv_assignment**)&r.assigns, &r.n_assigns, nullptr);
}

// --merge-on-gpu: the reads go up once; the other chunks receive them in HBM; every chunk runs; the collector merges
int PipelinedRun::call_merged(size_t wk, Work& w, CallResult& r) {
    mtsv_batch* ws = ws_[wk].get();
    std::vector<mtsv_batch*> cw;
    for (auto& b : cws_[wk]) cw.push_back(b.get());
    int rc = mtsv_batch_upload(cw[0], w.rb->bases.data(), w.rb->off.data(), w.rb->n());
    for (size_t c = 1; c < cw.size() && rc == MTSV_OK; c++) rc = mtsv_batch_copy_reads(cw[c], cw[0], nullptr);
    for (size_t c = 0; c < cw.size() && rc == MTSV_OK; c++) rc = mtsv_batch_run(cw[c], &p_);
    if (rc == MTSV_OK) rc = mtsv_batch_merge_runs(ws, cw.data(), (int)cw.size(), nullptr);
    if (rc == MTSV_OK) rc = cli_records_ ? download_records(ws, r) : mtsv_batch_download(ws, &r.hits, &r.n_hits);
    return rc;
}

// one index: the group's blocks in one call; behind --filter-index the chain -- what no filter matched goes down the stages
// and into the database's workspace, in HBM
int PipelinedRun::call_parts(size_t wk, Group& group, uint64_t group_reads, CallResult& r) {
    mtsv_batch* ws = ws_[wk].get();
    std::vector<const uint8_t*> pb;
    std::vector<const uint64_t*> po;
    std::vector<uint64_t> pn;
    for (auto& w : group) {
        pb.push_back(w->rb->bases.data());
        po.push_back(w->rb->off.data());
        pn.push_back(w->rb->n());
    }
    int rc = mtsv_batch_run_host_parts(filtered_ ? fws_[wk][0].get() : ws, (int)group.size(), pb.data(), po.data(), pn.data(), &p_);
    for (size_t k = 0; k < n_filters_ && rc == MTSV_OK; k++) {
        mtsv_batch* stage = fws_[wk][k].get();
        mtsv_batch* next = k + 1 < n_filters_ ? fws_[wk][k + 1].get() : ws;
        uint64_t kept = 0, kept_bases = 0, n_in = k ? 0 : group_reads;
        if (k) {
            mtsv_batch_stats st;
            rc = mtsv_batch_stats_get(stage, &st);
            n_in = st.n_reads;
        }
        if (rc == MTSV_OK) rc = mtsv_batch_take_reads(next, stage, MTSV_KEEP_UNMATCHED, &kept, &kept_bases, nullptr);
        if (rc == MTSV_OK) {
            stage_in_[k] += n_in;
            stage_removed_[k] += n_in - kept;
            rc = mtsv_batch_run(next, &p_);
        }
    }
    if (rc == MTSV_OK && cli_records_) rc = download_records(ws, r);
    else if (rc == MTSV_OK && match_mode_ != MTSV_MATCH_ONLY) rc = mtsv_batch_download(ws, &r.hits, &r.n_hits);  // (flags only: there are none)
    return rc;
}

// every batch gets its slice of the hits, read numbers relative to the batch
// (the boundaries by bisection, the renumbering on the formatting threads: a pass over a million hits between two
//  calls was 1.7 ms of every 8 the worker spent per megaread)
void PipelinedRun::hand_out(Group& group, const CallResult& r) {
    std::shared_ptr<void> owner(r.hits, [](void* q) { mtsv_hits_free((mtsv_hit*)q); });
    std::shared_ptr<void> a_owner(r.assigns, ArrayFree{});
    uint64_t first = 0, at = 0, a_at = 0;
    for (auto& w : group) {
        const uint64_t nr = w->rb->n();
        if (cli_records_) {
            uint64_t lo = a_at, hi = r.n_assigns;  // the first record of a later batch
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (record_read(r.assigns, mid) < first + nr) lo = mid + 1;
                else hi = mid;
            }
            w->assigns = r.assigns + a_at * a_rec_;
            w->n_assigns = lo - a_at;
            w->assigns_owner = a_owner;
            a_at = lo;
        }
        const uint64_t end = (uint64_t)(std::partition_point(r.hits + at, r.hits + r.n_hits, [&](const mtsv_hit& h) { return h.read < first + nr; }) - r.hits);
        w->hits = r.hits + at;
        w->n_hits = end - at;
        w->read_first = first;
        w->hits_owner = owner;
        w->flags = r.flags;
        at = end;
        first += nr;
    }
    for (auto& w : group) done_.push(std::move(w));
}

// one library call on a group of batches, and its results to the writer; on an error the code is set and the group dropped
void PipelinedRun::run_group(size_t wk, Group& group) {
    if (filtered_ && (group.size() == 1 && (group[0]->rb->bases.size() > chain_bases_ || group[0]->rb->n() > chain_reads_))) {
        code_.lib_error("a batch of reads holds more than " + std::to_string(chain_bases_) + " bases, which the workspaces behind a filter index were sized for: give a smaller --batch-reads");
        return;
    }
    uint64_t group_reads = 0;
    for (auto& w : group) group_reads += w->rb->n();
    InFlight in_flight(calls_in_flight_);
    const double t_g = now_s();
    CallResult r;
    int rc;
    if (merged_) {
        Work& w = *group[0];
        if (w.rb->n() > merge_reads_ || w.rb->bases.size() > merge_bases_) {
            code_.lib_error("a batch of reads holds more than " + std::to_string(merge_reads_) + " reads or " + std::to_string(merge_bases_) +
                            " bases, which the chunks' workspaces were sized for: give a smaller --batch-reads");
            return;
        }
        rc = call_merged(wk, w, r);
    } else if (chunked_) {
        Work& w = *group[0];
        std::vector<mtsv_index*> chunks;
        for (auto& ix : idx_) chunks.push_back(ix.get());
        rc = mtsv_bin_batch_chunks(chunks.data(), chunk_dev_.data(), (int)chunks.size(), w.rb->bases.data(), w.rb->off.data(), w.rb->n(), &p_, &r.hits, &r.n_hits);
    } else {
        rc = call_parts(wk, group, group_reads, r);
    }
    if (rc == MTSV_OK && partition_) {
        uint64_t *words = nullptr, n_flagged = 0, n_match = 0;
        rc = mtsv_batch_match_flags(ws_[wk].get(), &words, &n_flagged, &n_match);
        if (rc == MTSV_OK) {
            r.flags = std::shared_ptr<uint64_t>(words, ArrayFree{});
            reads_matched_ += n_match;
            if (n_flagged != group_reads) {
                code_.lib_error("match flags for " + std::to_string(n_flagged) + " reads, the call held " + std::to_string(group_reads));
                return;
            }
        }
    }
    if (rc != MTSV_OK) {
        code_.lib_error();
        return;
    }
    StageTimes::add(t_.gpu, now_s() - t_g);
    if (cli_timing_) {
        char what[96];
        snprintf(what, sizeof what, "worker %zu: call on %llu reads in %zu blocks took %.2f ms, ended", wk, (unsigned long long)group_reads,
                 group.size(), (now_s() - t_g) * 1e3);
        mark(what);
    }
    hand_out(group, r);
}

void PipelinedRun::gpu_worker(size_t wk) {
    for (;;) {
        const double t_p = now_s();
        Group group;
        if (chunked_) {
            group.push_back(parsed_.pop());
            if (!group[0]) break;
        } else {
            // a full group, or what there is when no call is running on any device (the start of the input, a slow parser)
            // (--filter-index: a call's reads must fit the chain's workspaces as one resident batch)
            group = parsed_.pop_group(group_reads_, group_max_, [&] { return calls_in_flight_.load() == 0; }, filtered_ ? chain_bases_ : ~0ull);
            if (group.empty()) break;
        }
        StageTimes::add(t_.gpu_wait, now_s() - t_p);
        if (code_.failed()) continue;  // drain
        run_group(wk, group);
    }
    mark("worker out of batches");
}

// the workers' counts add up: every read went through exactly one of their workspaces
bool PipelinedRun::gather_taxa(TaxaSum& sum) {
    for (auto& ws : ws_) {
        ArrayPtr<mtsv_taxon_stats> rows;
        uint64_t n_rows = 0, reads = 0;
        if (mtsv_batch_taxa_report(ws.get(), out(rows), &n_rows, &reads, nullptr, 0) != MTSV_OK) return false;
        if (!sum.add(std::move(rows), n_rows, reads)) return false;
    }
    return true;
}

void PipelinedRun::print_timing() const {
    if (!cli_timing_) return;
    fprintf(stderr, "[cli timing] batches %llu; reader: producing %.3f s, queue full %.3f s; gpu workers: in the library %.3f s, waiting for batches %.3f s; "
                    "writer: formatting %.3f s, waiting for hits %.3f s, waiting for the disk %.3f s\n",
            (unsigned long long)n_batches_, t_.ingest_wait.load() * 1e-6, t_.push_wait.load() * 1e-6, t_.gpu.load() * 1e-6, t_.gpu_wait.load() * 1e-6,
            t_.fmt.load() * 1e-6, t_.done_wait.load() * 1e-6, t_.write_wait.load() * 1e-6);
    if (getenv("MTSV_CLI_MARKS"))
        for (auto& m : marks_) fprintf(stderr, "[cli timing] %9.3f ms  %s\n", m.second * 1e3, m.first.c_str());
}

int PipelinedRun::run() {
    // (batches too large for one parser block are put together from several blocks by appending: those stay in ordinary
    //  memory -- growing a page-locked buffer means allocating another one -- and are staged by the library)
    std::thread stock_thread;
    JoinOnExit stock_joiner{stock_thread};
    if (install_pinned_blocks(run_.batch_reads)) {
        // stock: the parser's window of blocks plus what sits in the queues and with the workers
        const char* e = getenv("MTSV_INGEST_BLOCK");
        const uint64_t block_bytes = e ? strtoull(e, nullptr, 10) : 0;
        const uint64_t est = block_bytes ? block_bytes : run_.batch_reads * 320;
        const uint64_t per_call = std::min<uint64_t>(8, std::max<uint64_t>(1, std::max<uint64_t>(run_.batch_reads, 1ull << 20) / std::max<uint64_t>(run_.batch_reads, 1)));
        // (on a thread of its own: ~2 GB of page-locked memory take 0.1 s to create, the index is loaded meanwhile)
        const size_t n_stock = small_input_ ? 8 : std::min<size_t>(2 * host_threads_ + 2 + (size_t)(2 * per_call + 1) * (n_workers_ + 1), 128);
        const uint64_t stock_bytes = std::min<uint64_t>(est / 2 + (1 << 20), 512ull << 20);
        stock_thread = std::thread([this, n_stock, stock_bytes] { producer_.pool.stock(n_stock, stock_bytes); });
    }
    // The library would pack the bases to 4-bit codes on the host before they cross PCIe (host_pack.hpp: a dozen threads);
    // here the parser's threads need the CPUs and the link is not what bounds a run: the blocks go as they are
    // (MTSV_CLI_PACKED=1: packed).
    if (!getenv("MTSV_CLI_PACKED")) setenv("MTSV_H2D_PLAIN", "1", 0);
    // the two acceptance predicates are evaluated edit distance first (identical hits, about twice the device
    // rate for reads up to 253 bases); MTSV_VERIFY=reference keeps the reference's order
    if (!getenv("MTSV_VERIFY")) mtsv_set_default_verify_mode(MTSV_VERIFY_EDIT_FIRST);
    if (!load_indexes()) return code_.get();
    setup_mark("index loaded and resident");
    if (!make_workspaces()) return code_.get();
    setup_mark("workspaces ready");
    // parsed blocks land in page-locked memory from here on: the GPU copies them from where the parser put them
    if (stock_thread.joinable()) stock_thread.join();
    setup_mark("stock of page-locked blocks ready");
    logmsg("INFO", "Beginning queries.");
    t_begin_ = now_s();

    producer_.all_emitted = [this] {
        mark("last block parsed");
        parsed_.close();
    };
    std::thread reader([this] { read_input(); });
    // (the reader has handed on its last batch, or failed and said so, before the workers and the writer can end; what it
    //  may still be doing is closing its input -- unmapping 10 GB takes 45 ms -- and that is not part of the queries)
    JoinOnExit reader_join{reader};
    Helpers fmt_pool(host_threads_), write_pool(std::max(2u, host_threads_ / 2));
    std::thread writer([&] { write_output(fmt_pool, write_pool); });
    std::vector<std::thread> workers;
    for (size_t wk = 1; wk < n_workers_; wk++) workers.emplace_back([this, wk] { gpu_worker(wk); });
    gpu_worker(0);
    for (auto& t : workers) t.join();
    done_.close();
    writer.join();
    mark("writer done");
    if (code_.failed()) return code_.get();
    RunEnd end;
    end.t_begin = t_begin_;
    end.reads = reads_partitioned_.load();
    end.reads_matched = reads_matched_.load();
    end.info = [this] {
        for (size_t k = 0; k < n_filters_; k++)
            logmsg("INFO", "Filter stage " + std::to_string(k + 1) + " (" + run_.filter_paths[k] + "): removed " + std::to_string(stage_removed_[k].load()) + " of " +
                               std::to_string(stage_in_[k].load()) + " reads.");
    };
    TaxaSum taxa;
    end.taxa = &taxa;
    end.gather = [this](TaxaSum& sum) { return gather_taxa(sum); };
    end.mark = [this](const char* what) { mark(what); };
    if (const int c = finish(run_, out_, end)) return c;
    print_timing();
    setup_mark("queries done");
    // The results are on their way to the disk (close() has returned) and the log line is out: leave.  Handing 2 GB of
    // page-locked blocks, the workspaces and the resident index back piece by piece takes 0.3 s that the kernel's own
    // teardown of the process does not need (MTSV_CLI_CLEAN_EXIT=1: free everything, for leak checkers).
    if (!getenv("MTSV_CLI_CLEAN_EXIT")) {
        fflush(nullptr);  // (the reader thread may still be unmapping its input: it ends with the process)
        _exit(0);
    }
    ws_.clear();  // (30 ms per workspace: after the queries' clock, like the index)
    fws_.clear();
    cws_.clear();
    setup_mark("workspaces freed");
    idx_.clear();
    fidx_.clear();
    setup_mark("index freed");
    return 0;
}

}  // namespace

int run_pipelined(const Run& run, Producer& producer, Outputs& outputs) { return PipelinedRun(run, producer, outputs).run(); }

}  // namespace mtsv_cli
