// cons_rows_check.cpp -- the host-only side of mtsv_pileup_consensus (csrc/cons_rows.hpp: a row from a reference's cell, whether
// a reference is emitted, and the TSV of the rows) as a stand-alone program: built with the address and undefined-behaviour
// sanitizers and run on the CPU.  Edge values: an empty table, zero denominators, counts at 2^32 - 1, a sum of depths at
// 2^64 - 1, a TaxID of one row and one of several, the breadth threshold exactly met and missed by one part per million.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/cons_rows_check.cpp -o cons_rows_check
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../mtsv_tools_amd/csrc/cons_rows.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "FAILED: %s\n", what);
        failures++;
    }
}

bool has(const std::string& text, const char* line) { return text.find(line) != std::string::npos; }

}  // namespace

int main() {
    const std::string header = "taxid\tgi\tlength\tcovered\tbreadth_pct\tmean_depth\tcons_len\tref\tsub\tdel\tlow\tambiguous\tins_sites\tidentity_pct\n";
    expect(mtsv::format_consensus_stats(nullptr, 0) == header, "an empty table is the header alone");
    // ---- a row from a cell ----
    const uint32_t cell[10] = {600, 594, 5, 1, 3600, 0, 1, 0xdeadbeefu, 4711, 1};
    const mtsv_cons_ref r = mtsv::cons_row(7, 9, 4200, cell);
    expect(r.tax_id == 7 && r.gi == 9 && r.length == 4200 && r.covered == 600 && r.n_ref == 594 && r.n_sub == 5 && r.n_del == 1, "the cell's first counters");
    expect(r.n_low == 3600 && r.n_ambig == 0 && r.ins_sites == 1 && r.sum_depth == ((1ull << 32) | 4711), "the others; the pad is skipped");
    // ---- emitted ----
    mtsv_cons_ref e{};
    e.length = 64, e.covered = 16;
    expect(mtsv::cons_emitted(e, 250000) && !mtsv::cons_emitted(e, 250001) && mtsv::cons_emitted(e, 0), "a breadth of exactly 250000 ppm");
    e.covered = 0;
    expect(!mtsv::cons_emitted(e, 0), "no covered position: never emitted");
    e.length = e.covered = 0xffffffffu;
    expect(mtsv::cons_emitted(e, 1000000), "2^32 - 1 positions, all covered: the product stays inside 64 bits");
    // ---- the TSV ----
    const uint32_t top = 0xffffffffu;
    std::vector<mtsv_cons_ref> rows = {
        {1, 10, 4200, 600, 594, 5, 1, 3600, 0, 1, 4711},
        {1, 11, 3, 1, 0, 0, 0, 2, 1, 0, 2},
        {2, 20, 0, 0, 0, 0, 0, 0, 0, 1, 0},
        {7, 1, 9, 9, 0, 0, 9, 0, 0, 0, 36},
        {top, top, top, top, top, 0, 0, 0, 0, top, ~0ull},
    };
    const std::string text = mtsv::format_consensus_stats(rows.data(), rows.size());
    expect(text.rfind(header, 0) == 0, "the header first");
    expect(has(text, "\n1\t10\t4200\t600\t14.29\t1.12\t4199\t594\t5\t1\t3600\t0\t1\t99.00\n"), "a row");
    expect(has(text, "\n1\t11\t3\t1\t33.33\t0.67\t3\t0\t0\t0\t2\t1\t0\t0.00\n"), "nothing called: identity 0.00");
    expect(has(text, "\n1\t*\t4203\t601\t14.30\t1.12\t4202\t594\t5\t1\t3602\t1\t1\t99.00\n"), "the rollup takes the ratios of the sums");
    expect(has(text, "\n2\t20\t0\t0\t0.00\t0.00\t0\t0\t0\t0\t0\t0\t1\t0.00\n2\t*\t0\t0\t0.00\t0.00\t0\t0\t0\t0\t0\t0\t1\t0.00\n"), "a length of zero: every ratio 0.00");
    expect(has(text, "\n7\t1\t9\t9\t100.00\t4.00\t0\t0\t0\t9\t0\t0\t0\t0.00\n"), "deleted at every position: cons_len 0, identity 0.00");
    expect(has(text, "\n4294967295\t4294967295\t4294967295\t4294967295\t100.00\t4294967297.00\t4294967295\t4294967295\t0\t0\t0\t0\t4294967295\t100.00\n"),
           "counts of 2^32 - 1 and a sum of depths of 2^64 - 1");
    size_t n_lines = 0;
    for (char c : text) n_lines += c == '\n';
    expect(n_lines == 1 + rows.size() + 4, "a line per row and one per TaxID");
    if (failures) return 1;
    printf("cons_rows_check ok\n");
    return 0;
}
