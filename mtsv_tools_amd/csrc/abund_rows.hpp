// abund_rows.hpp -- the host-only side of mtsv_fold_abundance (abund.hip): the mismatch weights of mtsv_abundance_weights and the
// TSV of mtsv_format_abundance, over the row types of include/mtsv_amd.h.  Host code that includes nothing of HIP:
// tools/abund_rows_check.cpp builds it alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../include/mtsv_amd.h"

namespace mtsv {

static_assert(sizeof(mtsv_abundance_row) == 40, "the abundance row");
static_assert(sizeof(mtsv_abundance_info) == 48, "the abundance info");

constexpr uint32_t kAbundWeightsMax = 255;

// w[d - 1] = min(floor(q^d * 2^32), 2^32 - 1) for d = 1 .. n_w, the power by repeated multiplication; "arg: ..." unless
// 0 < q <= 1 (a NaN fails both compares) and 1 <= n_w <= 255
inline void abundance_weights(double q, uint32_t n_w, uint32_t* w) {
    if (!(q > 0.0) || !(q <= 1.0)) throw std::runtime_error("arg: the mismatch weight q is not in (0, 1]");
    if (n_w < 1 || n_w > kAbundWeightsMax) throw std::runtime_error("arg: a weight table of " + std::to_string(n_w) + " entries (1 .. 255)");
    double x = 1.0;
    for (uint32_t d = 1; d <= n_w; d++) {
        x = x * q;
        const double v = x * 4294967296.0;  // (exact: a power of two; at most 2^32, so the conversion below is defined)
        w[d - 1] = v >= 4294967295.0 ? 0xffffffffu : (uint32_t)(uint64_t)v;
    }
}

// header and one line per row: taxid, mass in reads (%.6f), abundance_pct of max(total_mass, 1) (%.4f), the three counts
inline std::string format_abundance(const mtsv_abundance_row* rows, uint64_t n_rows, const mtsv_abundance_info* info) {
    std::string text = "taxid\tmass\tabundance_pct\treads_any\treads_unique\tassigned\n";
    const uint64_t total = std::max<uint64_t>(info ? info->total_mass : 0, 1);
    char line[256];
    for (uint64_t i = 0; i < n_rows; i++) {
        const mtsv_abundance_row& r = rows[i];
        snprintf(line, sizeof line, "%u\t%.6f\t%.4f\t%llu\t%llu\t%llu\n", r.tax_id, (double)r.mass / 4294967296.0, (double)r.mass * 100.0 / (double)total,
                 (unsigned long long)r.reads_any, (unsigned long long)r.reads_unique, (unsigned long long)r.assigned);
        text += line;
    }
    return text;
}

}  // namespace mtsv
