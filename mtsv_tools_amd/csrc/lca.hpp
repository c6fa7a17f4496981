// lca.hpp -- what a fold keeps for mtsv_fold_lca (lca.hip): the device tree of its TaxIDs and the arrays of a call.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "taxonomy.hpp"

namespace mtsv {

// The part of a taxonomy a fold needs, numbered in preorder: the super-root (node 0, TaxID 0), the TaxIDs of the fold's union
// and all their ancestors; children ascending by TaxID.  A TaxID the taxonomy does not know is a child of the super-root.
struct LcaTree {
    std::vector<uint32_t> parent, last, tax, depth, rank;  // by node; parent[0] = 0
    std::vector<uint32_t> u_tax, u_node;                   // the union ascending, and its nodes
    uint32_t max_depth = 0;

    static LcaTree build(const Taxonomy& tx, const std::vector<uint32_t>& taxa);
    uint32_t nodes() const { return (uint32_t)tax.size(); }
};

// Created by a fold's first lca call, on the fold's stream.  The tree is rebuilt, and uploaded again, only when the union or
// the taxonomy has changed.
struct LcaState {
    int device;
    hipStream_t stream;  // the fold's
    bool timing = false;
    hipEvent_t ev[7] = {};
    LcaTree tree;
    uint64_t tree_serial = 0;         // the taxonomy's; 0: no tree yet
    std::vector<uint32_t> tree_taxa;  // the union it was built from
    uint32_t* d_tree = nullptr;       // parent, last, tax (n_nodes each), u_tax, u_node (n_union each)
    uint64_t tree_cap = 0;
    uint32_t *d_tile_cnt = nullptr, *d_tile_off = nullptr;
    uint64_t cnt_cap = 0, off_cap = 0;
    uint64_t* d_sums = nullptr;  // the scans' tile sums
    uint64_t sums_cap = 0;
    uint64_t* d_ctr = nullptr;  // kLcaCounters, then the two scans' totals
    uint64_t ctr_cap = 0;
    uint32_t* d_slot = nullptr;  // m, lo, hi: n_slots each
    uint64_t slot_cap = 0;
    uint32_t* d_node = nullptr;  // direct (n_nodes), prefix (n_nodes + 1), clade (n_nodes)
    uint64_t node_cap = 0;
    uint8_t* d_out = nullptr;  // the records of a call without an output fold
    uint64_t out_cap = 0;

    LcaState(int device, hipStream_t stream);
    ~LcaState();
    LcaState(const LcaState&) = delete;
    LcaState& operator=(const LcaState&) = delete;

    // MTSV_LCA_TILE as a tile size: a power of two, 64 .. kLcaTileMax; kLcaTile when it is not set
    static uint32_t tile_from_env();
};

}  // namespace mtsv
