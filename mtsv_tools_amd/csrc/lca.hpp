// lca.hpp -- what a fold keeps for mtsv_fold_lca (lca.hip): the device tree of its TaxIDs and the arrays of a call.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "dev_mem.hpp"
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
    DevEvents<7> ev;
    LcaTree tree;
    uint64_t tree_serial = 0;         // the taxonomy's; 0: no tree yet
    std::vector<uint32_t> tree_taxa;  // the union it was built from
    DevBuf<uint32_t> d_tree;          // parent, last, tax (n_nodes each), u_tax, u_node (n_union each)
    DevBuf<uint32_t> d_tile_cnt, d_tile_off;
    DevBuf<uint64_t> d_sums;  // the scans' tile sums
    DevBuf<uint64_t> d_ctr;   // kLcaCounters, then the two scans' totals
    DevBuf<uint32_t> d_slot;  // m, lo, hi: n_slots each
    DevBuf<uint32_t> d_node;  // direct (n_nodes), prefix (n_nodes + 1), clade (n_nodes)
    DevBuf<uint8_t> d_out;    // the records of a call without an output fold

    LcaState(int device, hipStream_t stream);
    ~LcaState();
    LcaState(const LcaState&) = delete;
    LcaState& operator=(const LcaState&) = delete;
};

}  // namespace mtsv
