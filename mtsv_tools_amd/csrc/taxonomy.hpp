// taxonomy.hpp -- an NCBI nodes.dmp as a tree on the host (taxonomy.cpp; mtsv_taxonomy, include/mtsv_amd.h).  Plain C++:
// no HIP and nothing else of the library, so that tools/taxonomy_check.cpp can build it alone under the sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace mtsv {

constexpr uint32_t kRankUnknown = 0xffffffffu;  // MTSV_RANK_UNKNOWN

// The listed nodes ascending by TaxID, the implied roots -- parents that have no line of their own -- beside them.  A node
// whose parent is itself is a root; every root and implied root hangs under the super-root, TaxID 0, which is no entry of
// either list.  Rank codes index rank_names, the file's distinct rank strings ascending by bytes.
struct Taxonomy {
    std::vector<uint32_t> ids, parents, ranks;  // one entry per listed node; parents[k] == ids[k] for a root
    std::vector<uint32_t> implied;              // ascending
    std::vector<std::string> rank_names;
    uint32_t max_depth = 0;  // the super-root is at depth 0, roots at 1
    uint64_t serial = 0;     // distinct for every taxonomy loaded by this process (what a cached device tree is keyed by)

    // Throws std::runtime_error: "io: ..." for a file that cannot be read, "format: ..." -- naming the line or the TaxID -- for
    // fewer than three fields, an ID that is not 1 to 10 digits up to 4294967295, TaxID 0, a TaxID listed twice, a cycle
    static Taxonomy load(const std::string& path);

    // the parent's TaxID (0 for roots, implied roots, the super-root and TaxIDs the file does not know) and the rank code;
    // false when tax_id is neither listed nor an implied root nor 0
    bool lookup(uint32_t tax_id, uint32_t* parent, uint32_t* rank) const;
    const char* rank_name(uint32_t rank) const { return rank < rank_names.size() ? rank_names[rank].c_str() : "-"; }
};

}  // namespace mtsv

struct mtsv_taxonomy {
    mtsv::Taxonomy impl;
};
