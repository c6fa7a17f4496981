// pile_refs_check -- the table of references of an mtsv_pileup by itself (csrc/pile_refs.hpp: the TaxID list, the plan of a call
// -- which bins are selected, which are known, which form the new segment and at which slots -- and the commit), with no device
// and no library, so that it can run under the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/pile_refs_check.cpp -o pile_refs_check
//   ./pile_refs_check
// An empty index, the TaxID list with duplicates, unsigned order, a chunk planned again, the same key with another length, one
// key in two bins, both limits, a hundred thousand references in two interleaving segments.  Prints one summary line; exit 2
// when a check fails.
#include <cstdio>
#include <cstdlib>

#include "../mtsv_tools_amd/csrc/pile_refs.hpp"

using mtsv::PileRefs;

#define REQUIRE(c)                                                       \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); \
            return 2;                                                    \
        }                                                                \
    } while (0)

static uint64_t key_of(uint32_t t, uint32_t g) { return (uint64_t)t << 32 | g; }

static std::string thrown(const PileRefs& r, const std::vector<uint64_t>& key, const std::vector<uint64_t>& len) {
    try {
        r.plan(key.data(), len.data(), key.size(), 0);
    } catch (const std::runtime_error& e) {
        return std::string(e.what()).substr(0, std::string(e.what()).find(':'));
    }
    return "";
}

// every invariant pile.hip relies on: ascending distinct keys, and inside a segment the slots laid end to end in key order
static bool sound(const PileRefs& r, uint32_t n_segs) {
    std::vector<uint64_t> next(n_segs, 0);
    for (size_t i = 0; i < r.refs.size(); i++) {
        if (i && r.refs[i - 1].key >= r.refs[i].key) return false;
        const PileRefs::Ref& x = r.refs[i];
        if (x.seg >= n_segs || x.off != next[x.seg]) return false;
        next[x.seg] += (uint64_t)x.len + 1;
    }
    return true;
}

int main() {
    PileRefs all;
    all.set_taxa(nullptr, 0);
    REQUIRE(all.selects(0) && all.selects(0xffffffffu) && all.n_slots() == 0 && all.find(key_of(1, 1)) == nullptr);
    {
        const PileRefs::Plan p = all.plan(nullptr, nullptr, 0, 0);
        REQUIRE(p.fresh.empty() && p.n_slots == 0 && p.bin_ref.empty());
        all.commit(p);
        REQUIRE(all.refs.empty());
    }
    // a first chunk: unsorted bins, a length of 0, a TaxID of 2^31 or more
    const std::vector<uint64_t> key = {key_of(9, 1), key_of(0x80000001u, 7), key_of(5, 3), key_of(5, 1)}, len = {64, 300, 0, 4200};
    PileRefs::Plan p = all.plan(key.data(), len.data(), key.size(), 0);
    REQUIRE(p.fresh.size() == 4 && p.n_slots == 65 + 301 + 1 + 4201);
    REQUIRE(p.fresh[0].key == key_of(5, 1) && p.fresh[0].off == 0 && p.fresh[1].key == key_of(5, 3) && p.fresh[1].off == 4201 && p.fresh[2].off == 4202);
    REQUIRE(p.fresh[3].key == key_of(0x80000001u, 7) && p.fresh[3].off == 4202 + 65);   // unsigned order: last
    REQUIRE(p.bin_ref[0] == -4 && p.bin_ref[1] == -5 && p.bin_ref[2] == -3 && p.bin_ref[3] == -2 && p.fresh_bin[0] == 3);
    REQUIRE(&PileRefs::of(p, all.refs, p.bin_ref[1]) == &p.fresh[3]);
    all.commit(p);
    REQUIRE(sound(all, 1) && all.refs.size() == 4 && all.n_slots() == p.n_slots && all.find(key_of(5, 3))->len == 0);
    // the chunk again, as another handle would bring it: nothing new, every bin finds its reference
    p = all.plan(key.data(), len.data(), key.size(), 1);
    REQUIRE(p.fresh.empty() && p.n_slots == 0 && p.bin_ref[0] == 2 && p.bin_ref[3] == 0 && PileRefs::of(p, all.refs, p.bin_ref[1]).key == key[1]);
    const std::vector<PileRefs::Ref> before = all.refs;
    all.commit(p);
    REQUIRE(all.refs.size() == before.size() && sound(all, 1));
    // refusals change nothing: another length, a key in two bins, both limits
    REQUIRE(thrown(all, {key_of(5, 1)}, {4199}) == "arg");
    REQUIRE(thrown(all, {key_of(6, 1), key_of(7, 1), key_of(6, 1)}, {10, 10, 10}) == "arg");
    REQUIRE(thrown(all, {key_of(6, 1)}, {0xffffffffull}) == "limit");
    REQUIRE(thrown(all, {key_of(6, 1), key_of(6, 2)}, {0x80000000ull, 0x7fffffffull}) == "limit");   // 2^32 + 1 slots
    REQUIRE(thrown(all, {key_of(6, 1), key_of(6, 2)}, {0x7ffffffeull, 0x7ffffffeull}) == "");      // 2^32 - 2
    REQUIRE(all.refs.size() == 4 && sound(all, 1));
    // a TaxID list: duplicates, unsorted; the others are unselected
    PileRefs some;
    const uint32_t taxa[] = {9, 5, 9, 0x80000001u};
    some.set_taxa(taxa, 4);
    REQUIRE(some.taxa.size() == 3 && some.selects(5) && !some.selects(6));
    const std::vector<uint64_t> key2 = {key_of(6, 1), key_of(5, 1), key_of(4, 4), key_of(9, 9)}, len2 = {7, 8, 9, 10};
    p = some.plan(key2.data(), len2.data(), key2.size(), 0);
    REQUIRE(p.fresh.size() == 2 && p.bin_ref[0] == PileRefs::Plan::kUnselected && p.bin_ref[2] == PileRefs::Plan::kUnselected && p.bin_ref[1] == -2 &&
            p.bin_ref[3] == -3 && p.n_slots == 9 + 11);
    some.commit(p);
    REQUIRE(thrown(some, {key_of(6, 1)}, {1ull << 40}) == "");   // (an unselected bin is not looked at)
    // a hundred thousand references in two segments whose keys interleave
    PileRefs big;
    big.set_taxa(nullptr, 0);
    const uint32_t n = 100000;
    for (uint32_t half = 0; half < 2; half++) {
        std::vector<uint64_t> k(n / 2), l(n / 2);
        for (uint32_t i = 0; i < n / 2; i++) {
            const uint32_t id = (2 * i + half) * 2654435761u;   // (odd multiplier: a permutation of the 32-bit numbers)
            k[i] = key_of(id >> 12, id & 0xfff);
            l[i] = id % 300;
        }
        p = big.plan(k.data(), l.data(), k.size(), half);
        REQUIRE(p.fresh.size() == n / 2);
        for (uint32_t i = 0; i < n / 2; i++) REQUIRE(PileRefs::of(p, big.refs, p.bin_ref[i]).key == k[i]);
        big.commit(p);
        REQUIRE(sound(big, half + 1) && big.refs.size() == (uint64_t)(half + 1) * (n / 2));
        p = big.plan(k.data(), l.data(), k.size(), half + 1);
        REQUIRE(p.fresh.empty());
        for (uint32_t i = 0; i < n / 2; i++) REQUIRE(p.bin_ref[i] >= 0 && big.refs[p.bin_ref[i]].key == k[i] && big.refs[p.bin_ref[i]].len == l[i]);
    }
    printf("pile_refs_check: ok (%zu, %zu and %zu references, %llu slots)\n", all.refs.size(), some.refs.size(), big.refs.size(),
           (unsigned long long)big.n_slots());
    return 0;
}
