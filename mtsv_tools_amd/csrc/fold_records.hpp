// fold_records.hpp -- the host-side check of records handed to mtsv_fold_add_records (fold.hip).  Plain C++, no HIP: a
// stand-alone program can run it under a sanitizer (tools/fold_records_check.cpp).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mtsv_amd.h"

namespace mtsv {

// Throws "arg: ..." unless the n records of `grain` at `records` have strictly ascending keys -- (read, tax_id); LONG (read,
// tax_id, gi, offset); TAXID_GI (read, tax_id, gi); unsigned -- and reads below n_reads.  taxa receives every record's tax_id
// (unsorted, with repeats).
inline void check_fold_records(int grain, const void* records, uint64_t n, uint64_t n_reads, std::vector<uint32_t>& taxa) {
    if (n && !records) throw std::runtime_error("arg: null records");
    taxa.clear();
    taxa.reserve(n);
    auto bad_order = [](uint64_t i) { return std::runtime_error("arg: record " + std::to_string(i) + " is not above its predecessor: keys must ascend strictly"); };
    auto bad_read = [n_reads](uint64_t i, uint64_t r) {
        return std::runtime_error("arg: record " + std::to_string(i) + " carries read " + std::to_string(r) + ", the fold was reset for " + std::to_string(n_reads) + " reads");
    };
    if (grain == MTSV_GRAIN_TAXID) {
        const auto* a = (const mtsv_assignment*)records;
        for (uint64_t i = 0; i < n; i++) {
            if (a[i].read >= n_reads) throw bad_read(i, a[i].read);
            if (i && !(a[i - 1].read < a[i].read || (a[i - 1].read == a[i].read && a[i - 1].tax_id < a[i].tax_id))) throw bad_order(i);
            taxa.push_back(a[i].tax_id);
        }
        return;
    }
    if (grain != MTSV_GRAIN_TAXID_GI && grain != MTSV_GRAIN_LONG) throw std::runtime_error("arg: bad assignment grain");
    const auto* a = (const mtsv_assignment_gi*)records;
    const bool with_offset = grain == MTSV_GRAIN_LONG;
    for (uint64_t i = 0; i < n; i++) {
        if (a[i].read >= n_reads) throw bad_read(i, a[i].read);
        if (i) {
            const mtsv_assignment_gi &p = a[i - 1], &q = a[i];
            const bool above = p.read != q.read ? p.read < q.read
                               : p.tax_id != q.tax_id ? p.tax_id < q.tax_id
                               : p.gi != q.gi       ? p.gi < q.gi
                                                    : with_offset && p.offset < q.offset;
            if (!above) throw bad_order(i);
        }
        taxa.push_back(a[i].tax_id);
    }
}

}  // namespace mtsv
