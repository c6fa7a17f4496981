// cover_refs_check -- the table of references of an mtsv_coverage by itself (csrc/cover_refs.hpp: bins into sorted unique
// (tax_id, gi, larger length), the word offsets, the "brings nothing new" test), with no device and no library, so that it can
// run under the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/cover_refs_check.cpp -o cover_refs_check
//   ./cover_refs_check
// Duplicates, lengths 0, 1 and 64, unsigned order, a million references, the re-add that is a no-op and the one that is
// longer, both limits.  Prints one summary line; exit 2 when a check fails.
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "../mtsv_tools_amd/csrc/cover_refs.hpp"

using mtsv::CoverRefs;

#define REQUIRE(c)                                                       \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); \
            return 2;                                                    \
        }                                                                \
    } while (0)

static std::vector<CoverRefs::Ref> refs_of(const std::vector<uint32_t>& t, const std::vector<uint32_t>& g, const std::vector<uint64_t>& l) {
    return CoverRefs::normalise(t.data(), g.data(), l.data(), t.size());
}

static bool limit_thrown(CoverRefs& table, const std::vector<uint32_t>& t, const std::vector<uint32_t>& g, const std::vector<uint64_t>& l) {
    try {
        table.merge(refs_of(t, g, l));
    } catch (const std::runtime_error& e) {
        return std::string(e.what()).rfind("limit:", 0) == 0;
    }
    return false;
}

// every invariant the kernels rely on
static bool sound(const CoverRefs& r) {
    if (r.len.size() != r.n() || r.word_off.size() != r.n() + 1 || r.word_off[0] != 0) return false;
    for (uint64_t i = 0; i < r.n(); i++) {
        if (i && r.key[i - 1] >= r.key[i]) return false;
        if (r.word_off[i + 1] - r.word_off[i] != CoverRefs::words_of(r.len[i])) return false;
    }
    return true;
}

int main() {
    CoverRefs table;
    REQUIRE(table.n() == 0 && table.words() == 0 && table.first_new({}) == nullptr);
    table.merge({});
    REQUIRE(table.n() == 0 && table.word_off.size() == 1 && sound(table));
    // duplicates in one call, lengths 0, 1, 64 and 65, a TaxID of 2^31 or more, unsorted input
    auto in = refs_of({9, 0x80000001u, 5, 5, 5, 9, 5, 5}, {1, 7, 3, 1, 2, 1, 1, 4}, {64, 300, 0, 1, 64, 10, 65, 1});
    REQUIRE(in.size() == 6);
    REQUIRE(table.first_new(in) == &in[0]);
    table.merge(in);
    REQUIRE(sound(table) && table.n() == 6);
    REQUIRE(table.key[0] == CoverRefs::key_of(5, 1) && table.len[0] == 65);   // the larger of 1 and 65
    REQUIRE(table.key[2] == CoverRefs::key_of(5, 3) && table.len[2] == 0 && table.word_off[2] == table.word_off[3]);
    REQUIRE(table.key[4] == CoverRefs::key_of(9, 1) && table.len[4] == 64);   // the larger of 64 and 10
    REQUIRE(table.key[5] == CoverRefs::key_of(0x80000001u, 7));               // unsigned order: last
    REQUIRE(table.words() == 2 + 1 + 0 + 1 + 1 + 5);
    REQUIRE(table.find(CoverRefs::key_of(5, 4)) == 3 && table.find(CoverRefs::key_of(5, 5)) == table.n());
    // the re-add that brings nothing new: the same, a part, shorter lengths
    REQUIRE(table.first_new(in) == nullptr);
    REQUIRE(table.first_new(refs_of({9, 5}, {1, 1}, {3, 65})) == nullptr);
    const CoverRefs before = table;
    table.merge(in);
    REQUIRE(table.key == before.key && table.len == before.len && table.word_off == before.word_off);
    // ... and the ones that do: a longer length, a new reference (the first of them is named)
    auto longer = refs_of({5, 9}, {1, 1}, {65, 65});
    REQUIRE(table.first_new(longer) == &longer[1]);
    auto fresh = refs_of({5, 4, 9}, {1, 9, 2}, {65, 7, 7});
    REQUIRE(table.first_new(fresh) == &fresh[0] && fresh[0].first == CoverRefs::key_of(4, 9));
    table.merge(longer);
    table.merge(fresh);
    REQUIRE(sound(table) && table.n() == 8 && table.len[table.find(CoverRefs::key_of(9, 1))] == 65 && table.find(CoverRefs::key_of(4, 9)) == 0);
    // both limits leave the table as it was
    const CoverRefs kept = table;
    bool thrown = false;
    try {
        refs_of({1}, {1}, {1ull << 32});
    } catch (const std::runtime_error& e) {
        thrown = std::string(e.what()).rfind("limit:", 0) == 0;
    }
    REQUIRE(thrown);
    {
        std::vector<uint32_t> t(65, 1), g(65);
        std::iota(g.begin(), g.end(), 1u);
        REQUIRE(limit_thrown(table, t, g, std::vector<uint64_t>(65, 0xffffffffull)));  // 65 * 2^26 words
        REQUIRE(table.key == kept.key && table.len == kept.len && table.word_off == kept.word_off);
        t.resize(63), g.resize(63);
        CoverRefs wide;
        wide.merge(refs_of(t, g, std::vector<uint64_t>(63, 0xffffffffull)));            // just below: 63 * 2^26
        REQUIRE(sound(wide) && wide.words() == 63ull << 26);
    }
    // a million references in two halves that interleave, then all of them again
    const uint32_t million = 1000000;
    std::vector<uint32_t> t(million / 2), g(million / 2);
    std::vector<uint64_t> l(million / 2);
    CoverRefs big;
    for (int half = 0; half < 2; half++) {
        for (uint32_t k = 0; k < million / 2; k++) {
            const uint32_t id = (2 * k + half) * 2654435761u;  // (odd multiplier: a permutation of the 32-bit numbers)
            t[k] = id >> 12;
            g[k] = id & 0xfff;
            l[k] = id % 200;
        }
        big.merge(refs_of(t, g, l));
        REQUIRE(sound(big) && big.n() == (uint64_t)(half + 1) * (million / 2));
    }
    REQUIRE(big.first_new(refs_of(t, g, l)) == nullptr);
    uint64_t words = 0;
    for (uint64_t i = 0; i < big.n(); i++) words += CoverRefs::words_of(big.len[i]);
    REQUIRE(words == big.words());
    l[7] += 1;
    REQUIRE(big.first_new(refs_of(t, g, l)) != nullptr);
    printf("cover_refs_check: ok (%llu and %llu references, %llu words)\n", (unsigned long long)table.n(), (unsigned long long)big.n(),
           (unsigned long long)big.words());
    return 0;
}
