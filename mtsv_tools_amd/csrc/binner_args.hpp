// binner_args.hpp -- mtsv-binner's command line: the flags as given (Args) and the run they describe (Run).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mtsv_amd.h"

namespace mtsv_cli {

struct Args {
    std::string fasta, fastq, index, results, report, matched, unmatched, filter_index, output_format = "default";
    std::string threads = "4", edit = "0.13", seed_size = "18", seed_interval = "15", min_seed = "0.015",
                max_hits = "2000", tune_max_hits = "200", max_assign, max_cand, read_offset = "0";
    bool verbose = false, force = false, parse_only = false, merge_gpu = false, fold_gpu = false, text_gpu = false, fold_prefetch = false, dedup = false;
    bool interleaved = false;                             // --interleaved: the input's records alternate mate 1 and mate 2
    std::string pair_mode, max_insert, unpaired_penalty;  // --pair-mode, --max-insert, --unpaired-penalty: "" when not given
    std::string coverage, coverage_slack;                 // --coverage, --coverage-slack: "" when not given
    std::string alignments;                               // --alignments: "" when not given
    std::string variants, variant_taxa, variant_slack, min_depth, min_alt_reads, min_alt_frac;  // --variants and its sub-flags: "" when not given
    // --consensus and its sub-flags: "" when not given
    std::string consensus, consensus_stats, consensus_min_depth, consensus_min_frac, consensus_min_breadth, consensus_fill, consensus_width;
    uint64_t fold_reads = 16ull << 20;  // --fold-reads: reads per super-batch of --fold-on-gpu (every chunk is loaded once per super-batch)
    std::vector<int> devices{0};
    uint64_t batch_reads = 1u << 17;  // parser blocks of ~40 MB; the GPU workers take up to 1 Mi reads of them per library call. End to end on 32 M reads: 64 Ki .., 128 Ki 70 M reads/s, 256 Ki 54, 512 Ki 37
};

// How the indexes and the devices are put together (the header comment of binner_main.cpp).
enum class Mode {
    single,      // one index, one device
    replicated,  // one index resident on every listed device
    chunks,      // --index a,b,..: chunk k on the k-th listed device, hits merged on the host
    merged,      // --merge-on-gpu: every chunk resident on one device
    folded,      // --fold-on-gpu: one chunk resident at a time
};

// A validated command line.  Nothing in it changes after resolve().
struct Run {
    std::string input;  // --fasta or --fastq
    bool fastq = false;
    mtsv_params params;
    unsigned host_threads = 1;  // -t sized the reference's worker pool; here: the host helper threads (parse, format)
    uint64_t read_offset = 0;   // --read-offset plus what a resumed run skips
    bool long_fmt = false;      // --output-format long
    std::string results, report, part_path[2];  // "" : not asked for; part_path: [0] --matched, [1] --unmatched
    bool append = false;                        // the results file exists and is resumed
    std::vector<std::string> index_paths, filter_paths;
    std::vector<int> devices;
    Mode mode = Mode::single;
    bool partition = false, filtered = false, parse_only = false;
    bool text_gpu = false, fold_prefetch = false, dedup = false;
    bool interleaved = false;              // reads 2p and 2p + 1 of the input are the mates of pair p
    int pair_mode = MTSV_PAIR_PROPER;      // --pair-mode
    uint32_t max_insert = 1000;            // --max-insert
    uint32_t unpaired_penalty = 0;         // --unpaired-penalty (--pair-mode either)
    std::string coverage;                  // --coverage: "" : not asked for
    uint32_t coverage_slack = 0;           // --coverage-slack: 0xffffffff for `all`
    std::string alignments;                // --alignments: "" : not asked for
    std::string variants;                  // --variants: "" : not asked for
    std::vector<uint32_t> variant_taxa;    // --variant-taxa: empty: every reference (of the run's one pileup: --variants, --consensus)
    uint32_t variant_slack = 0;            // --variant-slack: 0xffffffff for `all` (the same)
    uint32_t min_depth = 1, min_alt_reads = 1, min_alt_ppm = 0;  // --min-depth, --min-alt-reads, --min-alt-frac as parts per million
    std::string consensus, consensus_stats;  // --consensus, --consensus-stats: "" : not asked for
    uint32_t cons_min_depth = 1, cons_min_frac_ppm = 500000, cons_min_breadth_ppm = 0;  // --consensus-min-depth, -min-frac, -min-breadth
    uint32_t cons_fill = 0, cons_width = 60;                                            // --consensus-fill (0: n, 1: ref), --consensus-width
    uint64_t batch_reads = 0, fold_reads = 0;

    bool have_results() const { return !results.empty(); }
    bool have_report() const { return !report.empty(); }
    bool have_coverage() const { return !coverage.empty(); }
    bool have_alignments() const { return !alignments.empty(); }
    bool have_variants() const { return !variants.empty(); }
    bool have_consensus() const { return !consensus.empty(); }
    bool have_pileup() const { return have_variants() || have_consensus(); }  // one pileup per run, shared by the two
    bool merged() const { return mode == Mode::merged; }
    bool folded() const { return mode == Mode::folded; }
    bool chunked() const { return index_paths.size() > 1; }
};

[[noreturn]] void usage_error(const std::string& m);
// The flag loop.  --help and --version print and leave with 0, a usage error leaves with 1.
Args parse_args(int argc, char** argv);
// Validation, in the order that decides which message a doubly-wrong command line gets: flag combinations (exit 1), the
// numbers (panic, 101; the INFO / WARN lines of the parameters are logged on the way), the results path (3), the refusals
// to resume (1) and the resume scan (4).  Touches no file but the results file it may resume and the input it scans for that.
Run resolve(const Args& a);
// Checked once the output files are open, after "Deserializing candidate filter ...": an --index or --filter-index list
// that holds no path at all, "," for one (exit 1).
void require_index_paths(const Run& run);

}  // namespace mtsv_cli
