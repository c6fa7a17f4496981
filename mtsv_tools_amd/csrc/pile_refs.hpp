// pile_refs.hpp -- the reference table of a pileup (pile.hip; mtsv_pileup, include/mtsv_amd.h): which (tax_id, gi) it holds, in
// which segment and at which slot, and the plan of a call -- which bins of an index it selects, which of them are new.
// Host only, nothing of HIP: tools/pile_refs_check.cpp builds it alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace mtsv {

struct PileRefs {
    struct Ref {
        uint64_t key;   // tax_id << 32 | gi
        uint32_t len;   // bases: len + 1 slots
        uint32_t seg;   // the segment it lies in
        uint32_t off;   // its first slot there
    };
    std::vector<Ref> refs;        // ascending by key
    std::vector<uint32_t> taxa;   // ascending, distinct; empty: every reference

    void set_taxa(const uint32_t* t, uint64_t n) {
        taxa.assign(t, t + n);
        std::sort(taxa.begin(), taxa.end());
        taxa.erase(std::unique(taxa.begin(), taxa.end()), taxa.end());
        all = n == 0;
    }
    bool selects(uint32_t tax_id) const { return all || std::binary_search(taxa.begin(), taxa.end(), tax_id); }
    const Ref* find(uint64_t key) const {
        auto it = std::lower_bound(refs.begin(), refs.end(), key, [](const Ref& r, uint64_t k) { return r.key < k; });
        return it != refs.end() && it->key == key ? &*it : nullptr;
    }
    uint64_t n_slots() const {
        uint64_t n = 0;
        for (const Ref& r : refs) n += (uint64_t)r.len + 1;
        return n;
    }

    // What a call with an index of these bins does to the table.  Nothing is changed: commit() does that.
    struct Plan {
        static constexpr int64_t kUnselected = -1;
        std::vector<int64_t> bin_ref;  // per bin: kUnselected, k >= 0: refs[k], k <= -2: fresh[-k - 2]
        std::vector<Ref> fresh;        // the new segment's references, ascending by key, off filled in, seg = the next segment
        std::vector<uint32_t> fresh_bin;  // the bin each of them came from
        uint64_t n_slots = 0;          // of the new segment
    };
    // "arg: ..." for a (tax_id, gi) the table holds with another length, or that two of the bins carry; "limit: ..." for a
    // segment of 2^32 slots or more
    Plan plan(const uint64_t* key, const uint64_t* len, uint64_t n_bins, uint32_t next_seg) const {
        Plan p;
        p.bin_ref.assign(n_bins, Plan::kUnselected);
        std::vector<std::pair<uint64_t, uint32_t>> order;  // (key, bin) of the new ones
        for (uint64_t b = 0; b < n_bins; b++) {
            const uint32_t tax = (uint32_t)(key[b] >> 32);
            if (!selects(tax)) continue;
            if (const Ref* r = find(key[b])) {
                if (r->len != len[b])
                    throw std::runtime_error("arg: reference (tax_id " + std::to_string(tax) + ", gi " + std::to_string((uint32_t)key[b]) + ") has " +
                                             std::to_string(len[b]) + " bases in this index and " + std::to_string(r->len) + " in the pileup");
                p.bin_ref[b] = r - refs.data();
            } else {
                if (len[b] >= 0xffffffffull)
                    throw std::runtime_error("limit: reference (tax_id " + std::to_string(tax) + ", gi " + std::to_string((uint32_t)key[b]) + ") of " +
                                             std::to_string(len[b]) + " bases: a pileup segment holds fewer than 2^32 slots");
                order.emplace_back(key[b], (uint32_t)b);
            }
        }
        std::sort(order.begin(), order.end());
        for (size_t k = 0; k < order.size(); k++) {
            if (k && order[k].first == order[k - 1].first)
                throw std::runtime_error("arg: the index holds (tax_id " + std::to_string((uint32_t)(order[k].first >> 32)) + ", gi " +
                                         std::to_string((uint32_t)order[k].first) + ") in two bins");
            const uint64_t L = len[order[k].second];
            if (p.n_slots + L + 1 >= (1ull << 32))
                throw std::runtime_error("limit: the new references of this index take " + std::to_string(p.n_slots + L + 1) +
                                         " slots or more, 2^32 or more in one pileup segment: select fewer TaxIDs");
            p.fresh.push_back(Ref{order[k].first, (uint32_t)L, next_seg, (uint32_t)p.n_slots});
            p.fresh_bin.push_back(order[k].second);
            p.bin_ref[order[k].second] = -(int64_t)k - 2;
            p.n_slots += L + 1;
        }
        return p;
    }
    void commit(const Plan& p) {
        if (p.fresh.empty()) return;
        std::vector<Ref> both(refs.size() + p.fresh.size());
        std::merge(refs.begin(), refs.end(), p.fresh.begin(), p.fresh.end(), both.begin(), [](const Ref& a, const Ref& b) { return a.key < b.key; });
        refs.swap(both);
    }
    // the reference a plan's entry stands for (before or after commit: a plan's indexes are into the table it was made from)
    static const Ref& of(const Plan& p, const std::vector<Ref>& table, int64_t e) { return e >= 0 ? table[(size_t)e] : p.fresh[(size_t)(-e - 2)]; }

   private:
    bool all = true;
};

}  // namespace mtsv
