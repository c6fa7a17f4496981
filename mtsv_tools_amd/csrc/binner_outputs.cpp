// binner_outputs.cpp -- see binner_outputs.hpp
#include "binner_outputs.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <cstdio>

namespace mtsv_cli {

int Outputs::open(const Run& run) {
    if (run.have_results()) {
        out_fd = ::open(run.results.c_str(), O_WRONLY | O_CREAT | (run.append ? 0 : O_TRUNC), 0644);
        if (out_fd < 0) {
            logmsg("ERROR", "Error running query: cannot open results file " + run.results);
            return 2;
        }
        out_pos = lseek(out_fd, 0, SEEK_END);
    }
    for (int k = 0; k < 2; k++) {
        const std::string& path = run.part_path[k];
        if (path.empty()) continue;
        part_fd[k] = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (part_fd[k] < 0) {
            logmsg("ERROR", "Error running query: cannot open " + path);
            return 2;
        }
    }
    return 0;
}

bool TaxaSum::add(ArrayPtr<mtsv_taxon_stats> more, uint64_t n_more, uint64_t more_reads) {
    ArrayPtr<mtsv_taxon_stats> both;
    uint64_t n_both = 0;
    if (mtsv_merge_taxa_reports(rows.get(), n_rows, more.get(), n_more, out(both), &n_both) != MTSV_OK) return false;
    rows = std::move(both);
    n_rows = n_both;
    reads += more_reads;
    return true;
}

int finish(const Run& run, Outputs& outputs, const RunEnd& end) {
    auto mark = [&](const char* what) {
        if (end.mark) end.mark(what);
    };
    if (outputs.out_fd >= 0 && ::close(outputs.out_fd) != 0) {
        logmsg("ERROR", "Error writing to result file");
        return 11;
    }
    mark("results file closed");
    for (int k = 0; k < 2; k++)
        if (outputs.part_fd[k] >= 0 && ::close(outputs.part_fd[k]) != 0) {
            logmsg("ERROR", "Error writing to " + run.part_path[k]);
            return 11;
        }
    if (run.partition)
        logmsg("INFO", "Partitioned " + std::to_string(end.reads) + " reads: " + std::to_string(end.reads_matched) + " matched, " +
                           std::to_string(end.reads - end.reads_matched) + " unmatched.");
    if (end.info) end.info();
    if (run.have_report()) {
        ArrayPtr<char> text;
        uint64_t text_len = 0;
        if ((end.gather && !end.gather(*end.taxa)) ||
            mtsv_format_taxa_report(end.taxa->rows.get(), end.taxa->n_rows, end.taxa->reads, out(text), &text_len) != MTSV_OK) {
            logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
            return 2;
        }
        FILE* rf = fopen(run.report.c_str(), "wb");
        const bool written = rf && fwrite(text.get(), 1, text_len, rf) == text_len;
        if ((rf && fclose(rf) != 0) || !written) {
            logmsg("ERROR", "Error writing to taxa report file");
            return 11;
        }
        mark("taxa report written");
    }
    if (run.have_coverage()) {
        ArrayPtr<mtsv_ref_coverage> rows;
        ArrayPtr<char> text;
        uint64_t n_rows = 0, text_len = 0;
        int rc = end.coverage ? mtsv_coverage_rows(end.coverage, out(rows), &n_rows, nullptr) : MTSV_E_ARG;
        if (rc == MTSV_OK) rc = mtsv_format_coverage_report(rows.get(), n_rows, out(text), &text_len);
        if (rc != MTSV_OK) {
            logmsg("ERROR", std::string("Error running query: ") + (end.coverage ? mtsv_last_error() : "no coverage was counted"));
            return 2;
        }
        FILE* cf = fopen(run.coverage.c_str(), "wb");
        const bool written = cf && fwrite(text.get(), 1, text_len, cf) == text_len;
        if ((cf && fclose(cf) != 0) || !written) {
            logmsg("ERROR", "Error writing to coverage report file");
            return 11;
        }
        mark("coverage report written");
    }
    if (run.have_variants()) {
        ArrayPtr<mtsv_pile_site> rows;
        ArrayPtr<char> text;
        uint64_t n_rows = 0, text_len = 0;
        float ms = 0;
        int rc = end.pileup ? mtsv_pileup_sites(end.pileup, run.min_depth, run.min_alt_reads, run.min_alt_ppm, out(rows), &n_rows, &ms) : MTSV_E_ARG;
        if (rc == MTSV_OK) rc = mtsv_format_variants(rows.get(), n_rows, out(text), &text_len);
        if (rc != MTSV_OK) {
            logmsg("ERROR", std::string("Error running query: ") + (end.pileup ? mtsv_last_error() : "no pileup was counted"));
            return 2;
        }
        FILE* vf = fopen(run.variants.c_str(), "wb");
        const bool written = vf && fwrite(text.get(), 1, text_len, vf) == text_len;
        if ((vf && fclose(vf) != 0) || !written) {
            logmsg("ERROR", "Error writing to variants file");
            return 11;
        }
        if (end.variant_sites) *end.variant_sites = n_rows;
        if (end.variant_sites_ms) *end.variant_sites_ms = ms;
        mark("variant sites written");
    }
    if (run.have_consensus()) {  // the same accumulator, called once; the sites above have not changed it
        ArrayPtr<mtsv_cons_ref> rows;
        ArrayPtr<char> fasta, text;
        uint64_t n_rows = 0, fasta_len = 0, text_len = 0;
        float ms = 0;
        int rc = end.pileup ? mtsv_pileup_consensus(end.pileup, run.cons_min_depth, run.cons_min_frac_ppm, run.cons_min_breadth_ppm, run.cons_fill, run.cons_width,
                                                    out(fasta), &fasta_len, out(rows), &n_rows, &ms)
                            : MTSV_E_ARG;
        if (rc == MTSV_OK && !run.consensus_stats.empty()) rc = mtsv_format_consensus_stats(rows.get(), n_rows, out(text), &text_len);
        if (rc != MTSV_OK) {
            logmsg("ERROR", std::string("Error running query: ") + (end.pileup ? mtsv_last_error() : "no pileup was counted"));
            return 2;
        }
        FILE* ff = fopen(run.consensus.c_str(), "wb");
        bool written = ff && fwrite(fasta.get(), 1, fasta_len, ff) == fasta_len;
        if ((ff && fclose(ff) != 0) || !written) {
            logmsg("ERROR", "Error writing to consensus file");
            return 11;
        }
        if (!run.consensus_stats.empty()) {
            FILE* sf = fopen(run.consensus_stats.c_str(), "wb");
            written = sf && fwrite(text.get(), 1, text_len, sf) == text_len;
            if ((sf && fclose(sf) != 0) || !written) {
                logmsg("ERROR", "Error writing to consensus statistics file");
                return 11;
            }
        }
        if (end.consensus_refs) *end.consensus_refs = n_rows;
        if (end.consensus_bytes) *end.consensus_bytes = fasta_len;
        if (end.consensus_ms) *end.consensus_ms = ms;
        mark("consensus written");
    }
    char msg[160];
    snprintf(msg, sizeof msg, "All worker and result consumer threads terminated. Took %.3f seconds.", now_s() - end.t_begin);
    logmsg("INFO", msg);
    return 0;
}

}  // namespace mtsv_cli
