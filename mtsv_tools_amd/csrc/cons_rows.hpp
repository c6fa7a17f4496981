// cons_rows.hpp -- the host-only side of mtsv_pileup_consensus (cons.hip): a row from a reference's cell of counters, whether a
// reference is emitted, and the TSV of mtsv_format_consensus_stats, over the row type of include/mtsv_amd.h.  Host code that
// includes nothing of HIP: tools/cons_rows_check.cpp builds it alone under the sanitizers.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mtsv_amd.h"

namespace mtsv {

static_assert(sizeof(mtsv_cons_ref) == 48, "the consensus row");

// cell: covered, n_ref, n_sub, n_del, n_low, n_ambig, ins_sites, a pad, sum_depth as two words (k_cons.hip)
inline mtsv_cons_ref cons_row(uint32_t tax_id, uint32_t gi, uint32_t length, const uint32_t* cell) {
    mtsv_cons_ref r;
    memset(&r, 0, sizeof r);
    r.tax_id = tax_id, r.gi = gi, r.length = length;
    r.covered = cell[0], r.n_ref = cell[1], r.n_sub = cell[2], r.n_del = cell[3], r.n_low = cell[4], r.n_ambig = cell[5], r.ins_sites = cell[6];
    r.sum_depth = (uint64_t)cell[8] | (uint64_t)cell[9] << 32;
    return r;
}

inline bool cons_emitted(const mtsv_cons_ref& r, uint32_t min_breadth_ppm) {
    return r.covered >= 1 && (uint64_t)r.covered * 1000000ull >= (uint64_t)min_breadth_ppm * r.length;
}

// header, one line per row, and behind a TaxID's rows one line with gi `*`: the sums, and the three ratios of the sums
inline std::string format_consensus_stats(const mtsv_cons_ref* rows, uint64_t n_rows) {
    std::string text = "taxid\tgi\tlength\tcovered\tbreadth_pct\tmean_depth\tcons_len\tref\tsub\tdel\tlow\tambiguous\tins_sites\tidentity_pct\n";
    char line[400];
    // v: length, covered, ref, sub, del, low, ambiguous, ins_sites, sum_depth
    auto put = [&](uint32_t tax_id, const char* gi, const uint64_t* v) {
        const double breadth = v[0] ? (double)v[1] / (double)v[0] * 100.0 : 0.0, depth = v[0] ? (double)v[8] / (double)v[0] : 0.0;
        const uint64_t called = v[2] + v[3] + v[4];
        const double identity = called ? (double)v[2] / (double)called * 100.0 : 0.0;
        snprintf(line, sizeof line, "%u\t%s\t%llu\t%llu\t%.2f\t%.2f\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%.2f\n", tax_id, gi, (unsigned long long)v[0],
                 (unsigned long long)v[1], breadth, depth, (unsigned long long)(v[0] - v[4]), (unsigned long long)v[2], (unsigned long long)v[3],
                 (unsigned long long)v[4], (unsigned long long)v[5], (unsigned long long)v[6], (unsigned long long)v[7], identity);
        text += line;
    };
    for (uint64_t i = 0; i < n_rows;) {
        uint64_t j = i, sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (; j < n_rows && rows[j].tax_id == rows[i].tax_id; j++) {
            const mtsv_cons_ref& s = rows[j];
            const uint64_t v[9] = {s.length, s.covered, s.n_ref, s.n_sub, s.n_del, s.n_low, s.n_ambig, s.ins_sites, s.sum_depth};
            for (int k = 0; k < 9; k++) sum[k] += v[k];
            char gi[16];
            snprintf(gi, sizeof gi, "%u", s.gi);
            put(s.tax_id, gi, v);
        }
        put(rows[i].tax_id, "*", sum);
        i = j;
    }
    return text;
}

}  // namespace mtsv
