// cover_refs.hpp -- the table of references of an mtsv_coverage (cover.hip): sorted unique (tax_id, gi) with the larger length,
// the word offsets of the references' bitmaps, and the test "does this bring anything new".  Host code that includes nothing
// of HIP: tools/cover_refs_check.cpp builds it alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace mtsv {

struct CoverRefs {
    // a reference as it comes in: key = tax_id << 32 | gi (unsigned order of the pair), and its length
    using Ref = std::pair<uint64_t, uint64_t>;

    std::vector<uint64_t> key;       // ascending, distinct
    std::vector<uint32_t> len;       // below 2^32
    std::vector<uint32_t> word_off;  // n + 1: reference r owns the 64-bit words [word_off[r], word_off[r + 1]) of the bitmap

    uint64_t n() const { return key.size(); }
    uint64_t words() const { return word_off.empty() ? 0 : word_off.back(); }
    static uint64_t key_of(uint32_t tax_id, uint32_t gi) { return (uint64_t)tax_id << 32 | gi; }
    static uint64_t words_of(uint64_t length) { return (length + 63) / 64; }

    // the incoming references sorted, one per key with the larger length; "limit: ..." for a length of 2^32 or more
    static std::vector<Ref> normalise(const uint32_t* tax_id, const uint32_t* gi, const uint64_t* length, uint64_t n_in) {
        std::vector<Ref> in(n_in);
        for (uint64_t i = 0; i < n_in; i++) {
            if (length[i] >= (1ull << 32))
                throw std::runtime_error("limit: reference (tax_id " + std::to_string(tax_id[i]) + ", gi " + std::to_string(gi[i]) + ") is " +
                                         std::to_string(length[i]) + " bases long, 2^32 or more");
            in[i] = Ref(key_of(tax_id[i], gi[i]), length[i]);
        }
        std::sort(in.begin(), in.end());  // (equal keys: the larger length last)
        uint64_t m = 0;
        for (uint64_t i = 0; i < n_in; i++)
            if (i + 1 == n_in || in[i + 1].first != in[i].first) in[m++] = in[i];
        in.resize(m);
        return in;
    }

    // the place of a key, or n()
    uint64_t find(uint64_t k) const {
        const auto it = std::lower_bound(key.begin(), key.end(), k);
        return it != key.end() && *it == k ? (uint64_t)(it - key.begin()) : n();
    }

    // normalised references that the table does not hold yet, or holds with a smaller length: the first of them, or null
    const Ref* first_new(const std::vector<Ref>& in) const {
        uint64_t j = 0;
        for (const Ref& r : in) {
            while (j < n() && key[j] < r.first) j++;
            if (j == n() || key[j] != r.first || len[j] < r.second) return &r;
        }
        return nullptr;
    }

    // the table joined with normalised references; "limit: ..." when its bitmap would need 2^32 words or more, and then the
    // table is what it was
    void merge(const std::vector<Ref>& in) {
        std::vector<uint64_t> k2;
        std::vector<uint32_t> l2;
        k2.reserve(n() + in.size());
        l2.reserve(n() + in.size());
        uint64_t i = 0, j = 0, total = 0;
        while (i < n() || j < in.size()) {
            uint64_t k;
            uint32_t l;
            if (j == in.size() || (i < n() && key[i] < in[j].first)) {
                k = key[i];
                l = len[i++];
            } else if (i == n() || in[j].first < key[i]) {
                k = in[j].first;
                l = (uint32_t)in[j++].second;
            } else {
                k = key[i];
                l = std::max(len[i++], (uint32_t)in[j++].second);
            }
            k2.push_back(k);
            l2.push_back(l);
            total += words_of(l);
        }
        if (total >= (1ull << 32))
            throw std::runtime_error("limit: the bitmap of " + std::to_string(k2.size()) + " references would take " + std::to_string(total) +
                                     " 64-bit words, 2^32 or more");
        key.swap(k2);
        len.swap(l2);
        word_off.assign(n() + 1, 0);
        for (uint64_t r = 0; r < n(); r++) word_off[r + 1] = word_off[r] + (uint32_t)words_of(len[r]);
    }
};

}  // namespace mtsv
