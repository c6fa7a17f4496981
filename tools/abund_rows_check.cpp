// abund_rows_check.cpp -- the host-only side of mtsv_fold_abundance (csrc/abund_rows.hpp: the mismatch weights and the TSV of
// the rows) as a stand-alone program: built with the address and undefined-behaviour sanitizers and run on the CPU by
// tests/test_abundance_cpu.py.  Edge values: the ends of q, the table sizes 1 and 255, weights that underflow to zero, masses
// above 2^53 and at 2^64 - 1, a total mass of zero, an empty table.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/abund_rows_check.cpp -o abund_rows_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../mtsv_tools_amd/csrc/abund_rows.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        fprintf(stderr, "FAILED: %s\n", what);
        failures++;
    }
}

bool refused(double q, uint32_t n_w) {
    std::vector<uint32_t> w(256, 7);
    try {
        mtsv::abundance_weights(q, n_w, w.data());
    } catch (const std::runtime_error& e) {
        bool untouched = true;
        for (uint32_t v : w) untouched = untouched && v == 7;
        return untouched && std::string(e.what()).rfind("arg:", 0) == 0;
    }
    return false;
}

}  // namespace

int main() {
    // ---- weights ----
    for (uint32_t n_w : {1u, 2u, 64u, 255u}) {
        std::vector<uint32_t> w(n_w + 1, 0xabcdef01u);  // (one behind the table: it must stay)
        mtsv::abundance_weights(0.5, n_w, w.data());
        for (uint32_t d = 1; d <= n_w; d++) expect(w[d - 1] == (d <= 32 ? 1u << (32 - d) : 0u), "q = 0.5 gives 2^31, 2^30, ..., 1, 0, ...");
        expect(w[n_w] == 0xabcdef01u, "nothing is written behind the table");
        mtsv::abundance_weights(1.0, n_w, w.data());
        for (uint32_t d = 1; d <= n_w; d++) expect(w[d - 1] == 0xffffffffu, "q = 1 saturates at 2^32 - 1");
        mtsv::abundance_weights(1e-12, n_w, w.data());
        for (uint32_t d = 1; d <= n_w; d++) expect(w[d - 1] == 0, "q = 1e-12 is below 2^-32 from the first power on");
        mtsv::abundance_weights(std::nextafter(1.0, 0.0), n_w, w.data());
        expect(w[0] == 0xffffffffu, "the largest q below 1: floor((1 - 2^-53) * 2^32) = 2^32 - 1");
        mtsv::abundance_weights(std::numeric_limits<double>::denorm_min(), n_w, w.data());
        expect(w[0] == 0 && w[n_w - 1] == 0, "the smallest positive q");
        mtsv::abundance_weights(0.25, n_w, w.data());
        expect(w[0] == 1u << 30, "q = 0.25");
        for (uint32_t d = 2; d <= n_w; d++) expect(w[d - 1] <= w[d - 2], "weights do not grow with d");
    }
    expect(refused(0.0, 4) && refused(-0.5, 4) && refused(1.0000001, 4), "q outside (0, 1]");
    expect(refused(std::nan(""), 4) && refused(std::numeric_limits<double>::infinity(), 4), "NaN and infinity");
    expect(refused(0.5, 0) && refused(0.5, 256), "n_w outside 1 .. 255");
    // ---- the TSV ----
    const std::string header = "taxid\tmass\tabundance_pct\treads_any\treads_unique\tassigned\n";
    mtsv_abundance_info info{};
    expect(mtsv::format_abundance(nullptr, 0, &info) == header, "an empty table is the header alone");
    expect(mtsv::format_abundance(nullptr, 0, nullptr) == header, "... also without an info");
    const uint64_t top = ~0ull;
    std::vector<mtsv_abundance_row> rows = {
        {0, 0, 0, 0, 0, 0},
        {5, 0, 1ull << 32, 3, 1, 2},
        {7, 0, (1ull << 53) + 1, top, top, top},  // (a mass no double holds)
        {0xffffffffu, 0, top, 1, 0, 0},
    };
    info.total_mass = 1ull << 33;
    const std::string text = mtsv::format_abundance(rows.data(), rows.size(), &info);
    expect(text.rfind(header, 0) == 0, "the header first");
    expect(text.find("\n0\t0.000000\t0.0000\t0\t0\t0\n") != std::string::npos, "a row of zeros");
    expect(text.find("\n5\t1.000000\t50.0000\t3\t1\t2\n") != std::string::npos, "one read of two");
    expect(text.find("\n7\t2097152.000000\t104857600.0000\t18446744073709551615\t18446744073709551615\t18446744073709551615\n") != std::string::npos,
           "2^53 + 1 rounds to 2^53; counts of 2^64 - 1");
    expect(text.find("\n4294967295\t4294967296.000000\t214748364800.0000\t1\t0\t0\n") != std::string::npos, "a mass of 2^64 - 1 rounds to 2^64");
    info.total_mass = 0;  // (percentages of max(total_mass, 1))
    const std::string zero = mtsv::format_abundance(rows.data(), 2, &info);
    expect(zero.find("\n5\t1.000000\t429496729600.0000\t3\t1\t2\n") != std::string::npos, "a total mass of zero divides by one");
    size_t n_lines = 0;
    for (char c : text) n_lines += c == '\n';
    expect(n_lines == rows.size() + 1, "one line per row");
    if (failures) return 1;
    printf("abund_rows_check ok\n");
    return 0;
}
