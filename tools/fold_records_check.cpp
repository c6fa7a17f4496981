// fold_records_check.cpp -- the host-side check of mtsv_fold_add_records (csrc/fold_records.hpp) driven by a program of its
// own, so that it can run under a sanitizer on a machine without a GPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/fold_records_check.cpp -o fold_records_check && ./fold_records_check
// (on a hipcc line: -Xarch_host -fsanitize=address,undefined).  Exit status 0 and "fold_records_check ok" when every case
// behaves as stated; lists are heap arrays of exactly n records, so a read past the last one is the sanitizer's to report.
#include <cstdio>
#include <cstring>
#include <memory>

#include "../mtsv_tools_amd/csrc/fold_records.hpp"

namespace {
int failures = 0;

template <class R>
bool accepted(int grain, const std::vector<R>& recs, uint64_t n_reads, std::vector<uint32_t>* taxa_out = nullptr) {
    std::unique_ptr<R[]> heap(new R[recs.size()]);  // (exactly n records, no slack behind them)
    if (!recs.empty()) memcpy(heap.get(), recs.data(), recs.size() * sizeof(R));
    std::vector<uint32_t> taxa;
    try {
        mtsv::check_fold_records(grain, recs.empty() ? nullptr : heap.get(), recs.size(), n_reads, taxa);
    } catch (const std::runtime_error& e) {
        if (strncmp(e.what(), "arg:", 4) != 0) failures++, fprintf(stderr, "not an argument error: %s\n", e.what());
        return false;
    }
    if (taxa.size() != recs.size()) failures++, fprintf(stderr, "%zu TaxIDs for %zu records\n", taxa.size(), recs.size());
    if (taxa_out) *taxa_out = taxa;
    return true;
}
void expect(bool got, bool want, const char* what) {
    if (got != want) failures++, fprintf(stderr, "%s: %s, expected %s\n", what, got ? "accepted" : "refused", want ? "accepted" : "refused");
}
}  // namespace

int main() {
    using A = mtsv_assignment;
    using G = mtsv_assignment_gi;
    const uint32_t B = 0x80000000u;
    expect(accepted<A>(MTSV_GRAIN_TAXID, {}, 0), true, "empty list");
    expect(accepted<A>(MTSV_GRAIN_TAXID, {{0, 7, 1}, {0, B, 0}, {1, 3, 2}, {0xffffffffull + 5, 1, 1}}, 1ull << 33), true, "ascending, bit 31, reads beyond 2^32");
    expect(accepted<A>(MTSV_GRAIN_TAXID, {{0, B, 1}, {0, 7, 0}}, 4), false, "tax_id compared as signed would pass");
    expect(accepted<A>(MTSV_GRAIN_TAXID, {{0, 7, 1}, {0, 7, 0}}, 4), false, "a key twice");
    expect(accepted<A>(MTSV_GRAIN_TAXID, {{1, 7, 1}, {0, 9, 0}}, 4), false, "reads descending");
    expect(accepted<A>(MTSV_GRAIN_TAXID, {{0, 7, 1}, {4, 9, 0}}, 4), false, "read == n_reads");
    expect(accepted<A>(MTSV_GRAIN_TAXID, {{0, 7, 1}}, 0), false, "a record in a fold of no reads");
    const std::vector<G> pair = {{0, 7, 1, 4, 3}, {0, 7, 1, 9, 3}, {0, 7, B, 0, 1}, {2, 1, 1, 1, 1}};
    expect(accepted<G>(MTSV_GRAIN_LONG, pair, 3), true, "long: two offsets of one (tax_id, gi)");
    expect(accepted<G>(MTSV_GRAIN_TAXID_GI, pair, 3), false, "taxid-gi: the same pair twice");
    expect(accepted<G>(MTSV_GRAIN_LONG, {{0, 7, 1, 4, 3}, {0, 7, 1, 4, 2}}, 3), false, "long: a key twice");
    expect(accepted<G>(MTSV_GRAIN_LONG, {{0, 7, 1, 0xffffffffu, 3}, {0, 7, 2, 0, 2}}, 3), true, "long: gi decides before offset");
    expect(accepted<G>(MTSV_GRAIN_TAXID_GI, {{0, 7, 1, 4, 3}, {0, 7, B, 0, 2}, {1, 0, 0, 0, 0}}, 2), true, "taxid-gi ascending");
    expect(accepted<G>(MTSV_GRAIN_TAXID_GI, {{0, 7, 1, 4, 3}, {2, 7, 1, 4, 3}}, 2), false, "taxid-gi: read == n_reads");
    expect(accepted<G>(7, pair, 3), false, "a bad grain");
    std::vector<uint32_t> taxa;
    accepted<A>(MTSV_GRAIN_TAXID, {{0, 7, 1}, {1, 7, 2}, {1, 9, 2}}, 2, &taxa);
    if (taxa != std::vector<uint32_t>{7, 7, 9}) failures++, fprintf(stderr, "TaxIDs of the records are not handed back in order\n");
    if (failures) return 1;
    puts("fold_records_check ok");
    return 0;
}
