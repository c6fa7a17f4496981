// binner_fold.cpp -- the folded run of mtsv-binner, --fold-on-gpu: one chunk resident at a time.  A super-batch of reads is
// held on the host, in the (page-locked) blocks the parser filled, each block a PIECE with a fold of its own; per chunk: load,
// make resident, one workspace in MTSV_ASSIGN_ONLY, per piece upload + run + mtsv_fold_add_run, then the workspace and the
// index are freed.  After the last chunk a piece's records are its result lines (numbered from 0 within the piece, like its
// IDs: nothing to offset), its flags split its reads, its report adds to the run's.  Serial: this thread does all of it.
// --fold-prefetch: one loader thread runs mtsv_index_load of chunk c + 1 (after the last chunk: of chunk 0 for the next
// super-batch, when one is known to follow) while this thread makes chunk c resident, runs it over the pieces and folds.
// The chunks' uploads then pack on the device (MTSV_DEV_PACK_ON_DEVICE), which the measurement found 8 times faster.
// Depth 1: at most two host indexes are alive, and still one chunk is resident -- c + 1 goes up after c's workspace
// and index are freed.  mtsv_last_error is thread-local: the loader hands its message over with its return code, and
// a chunk that failed to load is reported when its turn comes.  flush() joins the loader on every way out.
// --dedup: a chunk's run sees the distinct sequences of a piece.  Per chunk and piece the reads go up into an intake
// workspace, mtsv_batch_take_unique packs the first read of every group of identical reads into the chunk's workspace,
// and the run is folded into the piece's fold of REPRESENTATIVES; after the last chunk mtsv_fold_expand fans those
// records out into the piece's fold proper, which everything else is derived from as without the flag.  The map is
// computed again for every chunk, into the piece's mtsv_dupmap, with the same content every time: hashing the piece
// once per chunk is the price of keeping no reads resident between chunks (a chunk's index may need that room).
// --interleaved: reads 2p and 2p + 1 of the input are the mates of pair p, so a piece holds an even number of reads: where a
// block of the parser ends on a mate 1, that read waits for the next block.  The reads are binned and folded as without the
// flag (at MTSV_GRAIN_LONG for --pair-mode proper, which needs the mates' GIs and offsets); after the last chunk, and after
// the expansion of --dedup, mtsv_fold_pair joins a piece's fold into its fold of PAIRS, which the result lines (one per
// pair, under the mates' common ID) and the report are derived from.
// --coverage: one mtsv_coverage for the whole run.  Every chunk that is loaded adds its bins to the table (from the second
// super-batch on that brings nothing new, which the library accepts); after the last chunk, and after the expansion of --dedup
// but before the pair join, a piece's fold of READS is added, the reads' lengths taken from the block's offsets.  The rows are
// asked for and written once, by finish().
// --alignments: after every run of a chunk over a piece, the hits the run left on the device are placed
// (mtsv_batch_place_hits with no hits given) and their lines, under the piece's read IDs, appended to the file: chunk by
// chunk, piece by piece.  Nothing else reads the placements, so every other output is what it is without the flag.
// --variants: one mtsv_pileup for the whole run.  After every run of a chunk over a piece, next to the placement of --alignments,
// the hits the run left on the device are piled (mtsv_pileup_add_run with no hits given: placed again, nothing comes to the
// host); a read's best edit is therefore its best in that chunk.  finish() asks for the sites once and writes them.
// --consensus: the same pileup -- one per run, made for either flag and shared by both -- called once by finish(), after the
// sites, which leave it as it was.
#include <fcntl.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "binner_run.hpp"

namespace mtsv_cli {
namespace {

// the loader thread's chunk
struct Prefetch {
    std::thread th;
    size_t chunk;  // the number of chunks when there is none
    IndexPtr ix;
    int rc = MTSV_OK;
    std::string err;
    double secs = 0;
    void start(size_t c, const std::string& path) {
        chunk = c;
        th = std::thread([this, path] {
            const double t0 = now_s();
            rc = mtsv_index_load(path.c_str(), out(ix));
            if (rc != MTSV_OK) err = mtsv_last_error();
            secs = now_s() - t0;
        });
    }
    void join() {
        if (th.joinable()) th.join();
    }
    ~Prefetch() { join(); }
};

struct JoinLoader {  // (no loader thread outlives flush())
    Prefetch& pre;
    ~JoinLoader() { pre.join(); }
};

class FoldedRun {
   public:
    FoldedRun(const Run& run, Producer& producer, Outputs& outputs)
        : run_(run), producer_(producer), out_(outputs), dev_(run.devices[0]),
          grain_(run.long_fmt || (run.interleaved && run.pair_mode == MTSV_PAIR_PROPER) ? MTSV_GRAIN_LONG : MTSV_GRAIN_TAXID),
          // (--interleaved: a piece may begin with the read the block before it ended on)
          piece_reads_(block_reads_max(run.batch_reads) + (run.interleaved ? 1 : 0)),
          piece_bases_(workspace_bases(piece_reads_, producer.warm_len(), 1 << 22)),
          // (... and a super-batch holds whole pairs)
          fold_reads_(run.interleaved ? std::max<uint64_t>(run.fold_reads & ~1ull, 2) : run.fold_reads) {
        pre_.chunk = run.index_paths.size();
    }
    int run();

   private:
    bool take_block(std::unique_ptr<ReadBlock> rb);
    bool take_pairs(std::unique_ptr<ReadBlock> rb);
    bool take_piece(std::unique_ptr<ReadBlock> rb);
    bool flush(bool more);  // the super-batch collected so far, through every chunk; more: another one follows
    bool make_folds();
    bool run_chunk(size_t c, bool more);
    bool write_piece(size_t k);
    bool write_results(const std::string& ids, const std::vector<uint64_t>& id_off, mtsv_fold* f);
    bool pair_piece(size_t k, const ReadBlock& rb, mtsv_fold* f);
    bool cover_piece(const ReadBlock& rb, mtsv_fold* f);
    bool align_piece(const ReadBlock& rb, mtsv_batch* ws);
    bool pile_piece(mtsv_batch* ws);
    bool input_error(const std::string& what);
    bool write_sides(const ReadBlock& rb, mtsv_fold* f);
    void print_timing() const;
    int leave(int c);

    const Run& run_;
    Producer& producer_;
    Outputs& out_;
    const int dev_, grain_;
    const uint64_t piece_reads_, piece_bases_, fold_reads_;
    ExitCode code_;
    Prefetch pre_;
    std::vector<std::unique_ptr<ReadBlock>> pieces_;
    std::vector<FoldPtr> folds_;  // one per piece of a super-batch, kept from super-batch to super-batch
    std::vector<FoldPtr> rep_folds_;  // --dedup: the folds of representatives, and the pieces' maps
    std::vector<DupmapPtr> dupmaps_;
    std::vector<FoldPtr> pair_folds_;    // --interleaved: the folds of pairs
    std::unique_ptr<ReadBlock> carry_;   // ... and a mate 1 whose mate 2 is the next block's first read
    std::string pair_ids_;               // the IDs of a piece's pairs, as a block holds its reads'
    std::vector<uint64_t> pair_id_off_;
    mtsv_pair_stats pair_stats_ = {0, 0, 0, 0, 0};
    uint64_t pairs_done_ = 0, reads_taken_ = 0;
    float pair_device_ms_ = 0;
    CoveragePtr coverage_;               // --coverage
    std::vector<uint32_t> read_len_;
    float coverage_device_ms_ = 0;
    int align_fd_ = -1;                  // --alignments
    uint64_t alignments_ = 0;
    float place_device_ms_ = 0;
    PileupPtr pileup_;                   // --variants, --consensus
    uint64_t piled_ = 0, pile_skipped_ = 0, variant_sites_ = 0, consensus_refs_ = 0, consensus_bytes_ = 0;
    float consensus_device_ms_ = 0;
    float pile_device_ms_ = 0, sites_device_ms_ = 0;
    TaxaSum taxa_;
    uint64_t dedup_reads_ = 0, dedup_distinct_ = 0;
    uint64_t super_reads_ = 0, n_super_ = 0, reads_done_ = 0, reads_matched_ = 0;
    double t_load_ = 0, t_resident_ = 0, t_run_ = 0, t_fold_ = 0, t_out_ = 0, t_loader_ = 0;
    float fold_device_ms_ = 0, text_device_ms_ = 0, dedup_device_ms_ = 0, expand_device_ms_ = 0;
};

bool FoldedRun::make_folds() {
    while (folds_.size() < pieces_.size()) {
        FoldPtr f;
        if (mtsv_fold_create(dev_, grain_, out(f)) != MTSV_OK) return code_.lib_error();
        folds_.push_back(std::move(f));
    }
    while (run_.dedup && rep_folds_.size() < pieces_.size()) {
        FoldPtr f;
        DupmapPtr m;
        if (mtsv_fold_create(dev_, grain_, out(f)) != MTSV_OK) return code_.lib_error();
        rep_folds_.push_back(std::move(f));
        if (mtsv_dupmap_create(dev_, out(m)) != MTSV_OK) return code_.lib_error();
        dupmaps_.push_back(std::move(m));
    }
    while (run_.interleaved && pair_folds_.size() < pieces_.size()) {
        FoldPtr f;
        if (mtsv_fold_create(dev_, MTSV_GRAIN_TAXID, out(f)) != MTSV_OK) return code_.lib_error();
        pair_folds_.push_back(std::move(f));
    }
    for (size_t k = 0; k < pieces_.size(); k++)
        if (mtsv_fold_reset((run_.dedup ? rep_folds_[k] : folds_[k]).get(), pieces_[k]->n()) != MTSV_OK) return code_.lib_error();
    return true;
}

// chunk c's turn: loaded (or taken from the loader), made resident, run over every piece and folded, freed
bool FoldedRun::run_chunk(size_t c, bool more) {
    const std::vector<std::string>& paths = run_.index_paths;
    IndexPtr ix;
    BatchPtr intake, ws;
    double t0 = now_s();
    int rc;
    if (run_.fold_prefetch && pre_.chunk == c) {  // the loader has it, or is on it: t_load counts the wait
        pre_.join();
        rc = pre_.rc;
        ix = std::move(pre_.ix);
        t_loader_ += pre_.secs;
        pre_.chunk = paths.size();
        if (rc != MTSV_OK) return code_.lib_error(pre_.err);
    } else {
        rc = mtsv_index_load(paths[c].c_str(), out(ix));
    }
    t_load_ += now_s() - t0;
    if (rc == MTSV_OK && coverage_) rc = mtsv_coverage_add_index(coverage_.get(), ix.get());
    if (run_.fold_prefetch && rc == MTSV_OK) {
        if (c + 1 < paths.size())
            pre_.start(c + 1, paths[c + 1]);
        else if (more)
            pre_.start(0, paths[0]);
    }
    t0 = now_s();
    // (under --fold-prefetch the chunk is packed on the device: 63 ms against 527 ms a chunk of 3.45e8 symbols,
    //  profiles/README.md r18; without the flag the upload is the one it was)
    if (rc == MTSV_OK) rc = mtsv_index_to_device(ix.get(), dev_, run_.fold_prefetch ? MTSV_DEV_PACK_ON_DEVICE : MTSV_DEV_DEFAULT);
    t_resident_ += now_s() - t0;
    if (rc == MTSV_OK) rc = mtsv_batch_create_lanes(ix.get(), dev_, piece_reads_, piece_bases_, 0, 1, out(ws));
    if (rc == MTSV_OK) rc = mtsv_batch_set_assignment_grain(ws.get(), grain_);
    if (rc == MTSV_OK) rc = mtsv_batch_set_assignments(ws.get(), MTSV_ASSIGN_ONLY);
    if (rc == MTSV_OK && run_.dedup) rc = mtsv_batch_create_lanes(ix.get(), dev_, piece_reads_, piece_bases_, 1, 1, out(intake));  // (it never runs)
    for (size_t k = 0; k < pieces_.size() && rc == MTSV_OK; k++) {
        const ReadBlock& rb = *pieces_[k];
        t0 = now_s();
        rc = mtsv_batch_upload(run_.dedup ? intake.get() : ws.get(), rb.bases.data(), rb.off.data(), rb.n());
        if (rc == MTSV_OK && run_.dedup) {
            uint64_t n_distinct = 0, bases_kept = 0;
            float ms = 0;
            rc = mtsv_batch_take_unique(ws.get(), intake.get(), dupmaps_[k].get(), &n_distinct, &bases_kept, &ms);
            dedup_device_ms_ += ms;
            if (rc == MTSV_OK && c == 0) {
                dedup_reads_ += rb.n();
                dedup_distinct_ += n_distinct;
            }
        }
        if (rc == MTSV_OK) rc = mtsv_batch_run(ws.get(), &run_.params);
        t_run_ += now_s() - t0;
        if (rc == MTSV_OK && align_fd_ >= 0 && !align_piece(rb, ws.get())) return false;
        if (rc == MTSV_OK && pileup_ && !pile_piece(ws.get())) return false;
        t0 = now_s();
        float ms = 0;
        if (rc == MTSV_OK) rc = mtsv_fold_add_run((run_.dedup ? rep_folds_[k] : folds_[k]).get(), ws.get(), &ms);
        fold_device_ms_ += ms;
        t_fold_ += now_s() - t0;
    }
    if (rc != MTSV_OK) return code_.lib_error();
    ws.reset();
    intake.reset();
    ix.reset();
    logmsg("DEBUG", "chunk " + paths[c] + " folded into " + std::to_string(pieces_.size()) + " pieces");
    return true;
}

// the input is not what the flags say it is: the exit code and the wording of a record the parser refuses (binner.rs:81-84)
bool FoldedRun::input_error(const std::string& what) {
    logmsg("ERROR", "Unable to read from input file: " + what);
    code_.set(12);
    return false;
}

// --interleaved: the piece's fold joined into its fold of pairs, and the pairs' IDs
bool FoldedRun::pair_piece(size_t k, const ReadBlock& rb, mtsv_fold* f) {
    pair_ids_.clear();
    pair_id_off_.assign(1, 0);
    for (uint64_t p = 0; 2 * p + 1 < rb.n(); p++) {
        const char *a = rb.ids.data() + rb.id_off[2 * p], *b = rb.ids.data() + rb.id_off[2 * p + 1];
        const size_t la = strlen(a), lb = strlen(b);
        size_t keep = la;
        if (la != lb || memcmp(a, b, la) != 0) {
            const bool stems = la == lb && la >= 2 && memcmp(a, b, la - 2) == 0 && a[la - 2] == '/' && a[la - 1] == '1' && b[la - 2] == '/' && b[la - 1] == '2';
            if (!stems)
                return input_error("the mates of pair " + std::to_string(run_.read_offset / 2 + pairs_done_ + p) + " of an interleaved input are named '" + a +
                                   "' and '" + b + "': neither one ID nor a stem with /1 and /2");
            keep = la - 2;
        }
        pair_ids_.append(a, keep);
        pair_ids_.push_back('\0');
        pair_id_off_.push_back(pair_ids_.size());
    }
    mtsv_pair_stats st;
    float ms = 0;
    if (mtsv_fold_pair(f, run_.pair_mode, run_.max_insert, run_.unpaired_penalty, pair_folds_[k].get(), &st, &ms) != MTSV_OK) return code_.lib_error();
    pair_device_ms_ += ms;
    pair_stats_.pairs += st.pairs;
    pair_stats_.both_mates_hit += st.both_mates_hit;
    pair_stats_.one_mate_hit += st.one_mate_hit;
    pair_stats_.joined += st.joined;
    pair_stats_.records += st.records;
    pairs_done_ += st.pairs;
    return true;
}

// --alignments: the hits of the run that has just ended on ws, placed and written under the piece's read IDs
bool FoldedRun::align_piece(const ReadBlock& rb, mtsv_batch* ws) {
    ArrayPtr<mtsv_placement> pl;
    ArrayPtr<uint32_t> ops;
    ArrayPtr<char> text;
    uint64_t n = 0, n_ops = 0, len = 0;
    float ms = 0;
    int rc = mtsv_batch_place_hits(ws, nullptr, 0, out(pl), &n, out(ops), &n_ops, &ms);
    if (rc == MTSV_OK) rc = mtsv_format_placements(pl.get(), n, ops.get(), rb.ids.data(), rb.id_off.data(), rb.n(), out(text), &len);
    if (rc != MTSV_OK) return code_.lib_error();
    place_device_ms_ += ms;
    alignments_ += n;
    if (!write_all(align_fd_, text.get(), len)) {
        logmsg("ERROR", "Error writing to alignments file");
        code_.set(11);
        return false;
    }
    return true;
}

// --variants: the hits of the run that has just ended on ws into the run's pileup
bool FoldedRun::pile_piece(mtsv_batch* ws) {
    uint64_t piled = 0, skipped = 0;
    float ms = 0;
    if (mtsv_pileup_add_run(pileup_.get(), ws, nullptr, 0, run_.variant_slack, &piled, &skipped, &ms) != MTSV_OK) return code_.lib_error();
    piled_ += piled;
    pile_skipped_ += skipped;
    pile_device_ms_ += ms;
    return true;
}

// --coverage: the piece's fold of reads into the run's accumulator
bool FoldedRun::cover_piece(const ReadBlock& rb, mtsv_fold* f) {
    read_len_.resize(rb.n());
    for (uint64_t i = 0; i < rb.n(); i++) read_len_[i] = (uint32_t)(rb.off[i + 1] - rb.off[i]);
    float ms = 0;
    if (mtsv_coverage_add_fold(coverage_.get(), f, read_len_.data(), rb.n(), run_.coverage_slack, &ms) != MTSV_OK) return code_.lib_error();
    coverage_device_ms_ += ms;
    return true;
}

bool FoldedRun::write_results(const std::string& ids, const std::vector<uint64_t>& id_off, mtsv_fold* f) {
    ArrayPtr<char> text;
    uint64_t len = 0;
    const uint64_t n_ids = id_off.size() - 1;
    int rc;
    if (run_.text_gpu) {  // (--text-on-gpu: the lines are written where the records are)
        float ms = 0;
        rc = mtsv_fold_format_text(f, ids.data(), id_off.data(), n_ids, out(text), &len, &ms);
        text_device_ms_ += ms;
    } else if (run_.long_fmt) {
        ArrayPtr<mtsv_assignment_gi> recs;
        uint64_t n_recs = 0;
        rc = mtsv_fold_download_gi(f, out(recs), &n_recs);
        if (rc == MTSV_OK) rc = mtsv_format_assignments_gi(recs.get(), n_recs, ids.data(), id_off.data(), n_ids, out(text), &len);
    } else {
        ArrayPtr<mtsv_assignment> recs;
        uint64_t n_recs = 0;
        rc = mtsv_fold_download(f, out(recs), &n_recs);
        if (rc == MTSV_OK) rc = mtsv_format_assignments(recs.get(), n_recs, ids.data(), id_off.data(), n_ids, out(text), &len);
    }
    if (rc != MTSV_OK) return code_.lib_error();
    if (!write_all(out_.out_fd, text.get(), len)) {
        logmsg("ERROR", "Error writing to result file");
        code_.set(11);
        return false;
    }
    return true;
}

// --matched / --unmatched: the piece's records, each to its side
bool FoldedRun::write_sides(const ReadBlock& rb, mtsv_fold* f) {
    ArrayPtr<uint64_t> words;
    uint64_t n_flagged = 0, n_match = 0;
    if (mtsv_fold_match_flags(f, out(words), &n_flagged, &n_match) != MTSV_OK) return code_.lib_error();
    std::string side[2];
    for (uint64_t i = 0; i < rb.n(); i++) {
        const int sd = (words.get()[i >> 6] >> (i & 63)) & 1 ? 0 : 1;
        if (out_.part_fd[sd] >= 0) mtsv_ingest::write_block_record(side[sd], run_.fastq, rb, i);
    }
    words.reset();
    reads_matched_ += n_match;
    for (int sd = 0; sd < 2; sd++)
        if (out_.part_fd[sd] >= 0 && !write_all(out_.part_fd[sd], side[sd].data(), side[sd].size())) {
            logmsg("ERROR", "Error writing to " + run_.part_path[sd]);
            code_.set(11);
            return false;
        }
    return true;
}

// after the last chunk: everything that is derived from piece k's records
bool FoldedRun::write_piece(size_t k) {
    const ReadBlock& rb = *pieces_[k];
    mtsv_fold* f = folds_[k].get();
    if (run_.dedup) {  // (the piece's map is the last chunk's, equal to every chunk's)
        float ms = 0;
        if (mtsv_fold_expand(f, rep_folds_[k].get(), dupmaps_[k].get(), &ms) != MTSV_OK) return code_.lib_error();
        expand_device_ms_ += ms;
    }
    if (coverage_ && !cover_piece(rb, f)) return false;
    if (run_.interleaved) {  // (from here on the piece is its pairs)
        if (!pair_piece(k, rb, f)) return false;
        f = pair_folds_[k].get();
    }
    if (out_.out_fd >= 0 && !(run_.interleaved ? write_results(pair_ids_, pair_id_off_, f) : write_results(rb.ids, rb.id_off, f))) return false;
    if (run_.have_report()) {
        ArrayPtr<mtsv_taxon_stats> rows;
        uint64_t n_rows = 0, reads = 0;
        if (mtsv_fold_taxa_report(f, out(rows), &n_rows, &reads, nullptr) != MTSV_OK) return code_.lib_error();
        if (!taxa_.add(std::move(rows), n_rows, reads)) return code_.lib_error();
    }
    if (run_.partition && !write_sides(rb, f)) return false;
    reads_done_ += rb.n();
    producer_.pool.put(std::move(pieces_[k]));
    return true;
}

bool FoldedRun::flush(bool more) {
    if (pieces_.empty()) return true;
    JoinLoader join_loader{pre_};
    if (!make_folds()) return false;
    for (size_t c = 0; c < run_.index_paths.size(); c++)
        if (!run_chunk(c, more)) return false;
    const double t0 = now_s();
    for (size_t k = 0; k < pieces_.size(); k++)
        if (!write_piece(k)) return false;
    t_out_ += now_s() - t0;
    pieces_.clear();
    super_reads_ = 0;
    n_super_++;
    logmsg("DEBUG", "taxonomic binning: " + std::to_string(reads_done_) + " reads done");
    return true;
}

bool FoldedRun::take_piece(std::unique_ptr<ReadBlock> rb) {
    if (rb->n() > piece_reads_ || rb->bases.size() > piece_bases_)
        return code_.lib_error("a batch of reads holds more than " + std::to_string(piece_reads_) + " reads or " + std::to_string(piece_bases_) +
                               " bases, which the chunks' workspaces are sized for: give a smaller --batch-reads");
    if (!pieces_.empty() && super_reads_ + rb->n() > fold_reads_ && !flush(true)) return false;
    super_reads_ += rb->n();
    reads_taken_ += rb->n();
    pieces_.push_back(std::move(rb));
    return true;
}

// a block of the parser, cut where it holds more than a super-batch
bool FoldedRun::take_block(std::unique_ptr<ReadBlock> rb) {
    // (the parser hands out blocks of up to one and a half batches: a super-batch holds at most --fold-reads reads)
    if (rb->n() <= fold_reads_) return take_piece(std::move(rb));
    for (uint64_t from = 0; from < rb->n(); from += fold_reads_) {
        auto part = producer_.pool.get();
        part->append(*rb, from, std::min<uint64_t>(from + fold_reads_, rb->n()));
        if (!take_piece(std::move(part))) return false;
    }
    producer_.pool.put(std::move(rb));
    return true;
}

// --interleaved: the read a block ended on goes in front of the next block, and a block that ends on a mate 1 gives it up
bool FoldedRun::take_pairs(std::unique_ptr<ReadBlock> rb) {
    const bool carried = carry_ && carry_->n();
    if (!carried && !(rb->n() & 1)) return take_block(std::move(rb));
    auto part = producer_.pool.get();
    if (carried) part->append(*carry_);
    const uint64_t whole = rb->n() - ((part->n() + rb->n()) & 1);
    part->append(*rb, 0, whole);
    if (!carry_) carry_.reset(new ReadBlock);
    carry_->clear();
    carry_->append(*rb, whole);
    producer_.pool.put(std::move(rb));
    if (!part->n()) {
        producer_.pool.put(std::move(part));
        return true;
    }
    return take_block(std::move(part));
}

// MTSV_CLI_TIMING=1: where a folded run spends its time (seconds; tools/fold_ab.py reads this line)
// (--fold-prefetch: index_load is the time this thread waited for the loader -- and the first chunk's load -- and the
//  loader's own time, which ran beside the other figures, follows)
void FoldedRun::print_timing() const {
    if (!getenv("MTSV_CLI_TIMING")) return;
    char prefetch_note[96] = "";
    if (run_.fold_prefetch) snprintf(prefetch_note, sizeof prefetch_note, "; prefetch: loader %.3f s, waited_for_loader %.3f s", t_loader_, t_load_);
    fprintf(stderr, "[cli fold timing] super_batches %llu chunks %zu reads %llu; index_load %.3f s, index_to_device %.3f s, upload_and_run %.3f s, fold %.3f s "
                    "(device %.3f ms), results_report_flags %.3f s%s\n",
            (unsigned long long)n_super_, run_.index_paths.size(), (unsigned long long)reads_done_, t_load_, t_resident_, t_run_, t_fold_, fold_device_ms_, t_out_,
            prefetch_note);
    if (run_.text_gpu) fprintf(stderr, "[cli text timing] text_on_gpu device %.3f ms\n", text_device_ms_);
    if (run_.dedup) fprintf(stderr, "[cli dedup timing] take_unique device %.3f ms, expand device %.3f ms\n", dedup_device_ms_, expand_device_ms_);
    if (run_.interleaved) fprintf(stderr, "[cli pair timing] pair device %.3f ms\n", pair_device_ms_);
    if (run_.have_coverage()) fprintf(stderr, "[cli coverage timing] coverage device %.3f ms\n", coverage_device_ms_);
    if (run_.have_alignments()) fprintf(stderr, "[cli alignments timing] alignments %llu, place device %.3f ms\n", (unsigned long long)alignments_, place_device_ms_);
    if (run_.have_variants())
        fprintf(stderr, "[cli variants timing] hits piled %llu, skipped %llu, sites %llu; place and pile device %.3f ms, sites device %.3f ms\n",
                (unsigned long long)piled_, (unsigned long long)pile_skipped_, (unsigned long long)variant_sites_, pile_device_ms_, sites_device_ms_);
    if (run_.have_consensus())
        fprintf(stderr, "[cli consensus timing] hits piled %llu, skipped %llu, references %llu, bytes %llu; place and pile device %.3f ms, consensus device %.3f ms\n",
                (unsigned long long)piled_, (unsigned long long)pile_skipped_, (unsigned long long)consensus_refs_, (unsigned long long)consensus_bytes_,
                pile_device_ms_, consensus_device_ms_);
}

// every way out of the folded run ends alike: the process leaves at once, or (MTSV_CLI_CLEAN_EXIT=1) frees what it holds --
// the folds, the maps and a chunk the loader brought for a super-batch that never came, as this object goes
int FoldedRun::leave(int c) {
    pre_.join();  // (joined by flush() already)
    if (!getenv("MTSV_CLI_CLEAN_EXIT")) {
        fflush(nullptr);
        _exit(c);
    }
    return c;
}

int FoldedRun::run() {
    install_pinned_blocks(run_.batch_reads);
    if (!getenv("MTSV_VERIFY")) mtsv_set_default_verify_mode(MTSV_VERIFY_EDIT_FIRST);
    logmsg("INFO", "Beginning queries.");
    const double t_begin = now_s();
    if (run_.have_coverage() && mtsv_coverage_create(dev_, out(coverage_)) != MTSV_OK) {
        code_.lib_error();
        return leave(code_.get());
    }
    if (run_.have_pileup() &&
        mtsv_pileup_create(dev_, run_.variant_taxa.empty() ? nullptr : run_.variant_taxa.data(), run_.variant_taxa.size(), out(pileup_)) != MTSV_OK) {
        code_.lib_error();
        return leave(code_.get());
    }
    if (run_.have_alignments()) {
        align_fd_ = ::open(run_.alignments.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (align_fd_ < 0) {
            logmsg("ERROR", "Error running query: cannot open alignments file " + run_.alignments);
            return leave(2);
        }
    }
    const bool parsed = producer_.produce(std::min<uint64_t>(run_.batch_reads, fold_reads_), [&](std::unique_ptr<ReadBlock> rb) {
        return run_.interleaved ? take_pairs(std::move(rb)) : take_block(std::move(rb));
    });
    if (!parsed && !code_.failed()) {
        logmsg("ERROR", "Unable to read from input file: " + producer_.error());
        code_.set(12);  // binner.rs:81-84
    }
    if (!code_.failed() && carry_ && carry_->n())
        input_error("an interleaved input of an odd number of records: record " + std::to_string(run_.read_offset + reads_taken_) + " ('" +
                    carry_->ids.c_str() + "') has no mate");
    if (!code_.failed()) flush(false);
    if (code_.failed()) return leave(code_.get());
    if (align_fd_ >= 0 && ::close(align_fd_) != 0) {
        logmsg("ERROR", "Error writing to alignments file");
        return leave(11);
    }
    RunEnd end;
    end.t_begin = t_begin;
    end.reads = reads_done_;
    end.reads_matched = reads_matched_;
    end.info = [&] {
        if (run_.dedup) logmsg("INFO", "Collapsed " + std::to_string(dedup_reads_) + " reads to " + std::to_string(dedup_distinct_) + " distinct sequences.");
        if (run_.interleaved)
            logmsg("INFO", "Joined " + std::to_string(pair_stats_.pairs) + " pairs: both mates hit " + std::to_string(pair_stats_.both_mates_hit) + ", one mate hit " +
                               std::to_string(pair_stats_.one_mate_hit) + ", joined " + std::to_string(pair_stats_.joined) + ".");
    };
    end.taxa = &taxa_;
    end.coverage = coverage_.get();
    end.pileup = pileup_.get();
    end.variant_sites = &variant_sites_;
    end.variant_sites_ms = &sites_device_ms_;
    end.consensus_refs = &consensus_refs_;
    end.consensus_bytes = &consensus_bytes_;
    end.consensus_ms = &consensus_device_ms_;
    if (const int c = finish(run_, out_, end)) return leave(c);
    print_timing();
    return leave(0);
}

}  // namespace

int run_folded(const Run& run, Producer& producer, Outputs& outputs) { return FoldedRun(run, producer, outputs).run(); }

}  // namespace mtsv_cli
