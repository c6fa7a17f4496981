// binner_outputs.hpp -- the files a run of mtsv-binner writes, and the end that both kinds of run share.
#pragma once
#include <sys/types.h>

#include <functional>

#include "binner_args.hpp"
#include "binner_handles.hpp"

namespace mtsv_cli {

// The results file and the partition files ([0] matched, [1] unmatched); -1: not asked for.  Written at positions the
// writers keep here (positional writes from several threads), or appended to in order.
struct Outputs {
    int out_fd = -1;
    off_t out_pos = 0;
    int part_fd[2] = {-1, -1};
    off_t part_pos[2] = {0, 0};
    // Creates the files: the results file truncated unless the run resumes it, the partition files truncated.  0, or the
    // exit code (logged).
    int open(const Run& run);
};

// Per-TaxID read counts, summed over the workspaces or folds they were counted in.
struct TaxaSum {
    ArrayPtr<mtsv_taxon_stats> rows;
    uint64_t n_rows = 0, reads = 0;
    // adds a report and takes it over; false: mtsv_last_error() says why
    bool add(ArrayPtr<mtsv_taxon_stats> more, uint64_t n_more, uint64_t more_reads);
};

// What a run hands to finish().
struct RunEnd {
    double t_begin = 0;                       // now_s() at "Beginning queries."
    uint64_t reads = 0, reads_matched = 0;    // --matched / --unmatched: for the "Partitioned" line
    std::function<void()> info;               // the run's own INFO lines, after that one
    TaxaSum* taxa = nullptr;                  // --report: the counts ...
    std::function<bool(TaxaSum&)> gather;     // ... or what still has to be added to them (false: a library error)
    mtsv_coverage* coverage = nullptr;        // --coverage: the run's accumulator
    mtsv_pileup* pileup = nullptr;            // --variants, --consensus: the run's one accumulator
    uint64_t* variant_sites = nullptr;        // ... where finish() leaves the number of sites it wrote, and the device time
    float* variant_sites_ms = nullptr;
    uint64_t* consensus_refs = nullptr;       // --consensus: the references and bytes finish() wrote, and the device time
    uint64_t* consensus_bytes = nullptr;
    float* consensus_ms = nullptr;
    std::function<void(const char*)> mark;    // MTSV_CLI_TIMING: a phase has ended
};
// The end of a run whose reads are all through: closes the results file and the partition files, logs the "Partitioned"
// line and the run's own, writes the taxa report, the coverage report, the variant sites and the consensus, logs "Took ... seconds.".  0, or the exit code
// (logged).
int finish(const Run& run, Outputs& outputs, const RunEnd& end);

}  // namespace mtsv_cli
