// lca.hip -- mtsv_fold_lca (include/mtsv_amd.h): the device tree of a fold's TaxIDs, built on the host from a taxonomy, and the
// five steps of k_lca.hip over the fold's records.  What comes down is counters and two words per node of the tree; the
// records of the reads' LCAs stay in HBM, in the output fold.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <stdexcept>
#include <string>

#include "fold.hpp"
#include "lca.hpp"

namespace mtsv {

LcaTree LcaTree::build(const Taxonomy& tx, const std::vector<uint32_t>& taxa) {
    // ---- the TaxIDs of the tree below the super-root: the union and, level by level, the parents not met yet ----
    std::vector<uint32_t> all, frontier, next, fresh, merged;
    for (uint32_t t : taxa)
        if (t) all.push_back(t);  // (ascending and distinct, as the fold keeps them)
    frontier = all;
    while (!frontier.empty()) {
        next.clear();
        for (uint32_t t : frontier) {
            uint32_t p, r;
            tx.lookup(t, &p, &r);
            if (p) next.push_back(p);
        }
        std::sort(next.begin(), next.end());
        next.erase(std::unique(next.begin(), next.end()), next.end());
        fresh.clear();
        std::set_difference(next.begin(), next.end(), all.begin(), all.end(), std::back_inserter(fresh));
        merged.resize(all.size() + fresh.size());
        std::merge(all.begin(), all.end(), fresh.begin(), fresh.end(), merged.begin());
        all.swap(merged);
        frontier.swap(fresh);
    }
    const size_t n_below = all.size();
    if (n_below + 1 >= (1ull << 31)) throw std::runtime_error("limit: a device tree of 2^31 nodes or more");
    std::vector<uint32_t> up(n_below), rk(n_below);  // parent TaxID (0: the super-root), rank code
    for (size_t k = 0; k < n_below; k++) tx.lookup(all[k], &up[k], &rk[k]);
    // ---- children ascending by TaxID under every parent: the places ordered by (parent, TaxID) ----
    std::vector<uint32_t> by_parent(n_below);
    for (size_t k = 0; k < n_below; k++) by_parent[k] = (uint32_t)k;
    std::stable_sort(by_parent.begin(), by_parent.end(), [&](uint32_t a, uint32_t b) { return up[a] < up[b]; });
    auto children = [&](uint32_t parent_tax, size_t* b, size_t* e) {
        *b = (size_t)(std::lower_bound(by_parent.begin(), by_parent.end(), parent_tax, [&](uint32_t k, uint32_t t) { return up[k] < t; }) - by_parent.begin());
        *e = (size_t)(std::upper_bound(by_parent.begin(), by_parent.end(), parent_tax, [&](uint32_t t, uint32_t k) { return t < up[k]; }) - by_parent.begin());
    };
    // ---- preorder: a stack of places, the children pushed largest first ----
    LcaTree T;
    const size_t N = n_below + 1;
    T.parent.assign(N, 0);
    T.last.assign(N, 0);
    T.tax.assign(N, 0);
    T.depth.assign(N, 0);
    T.rank.assign(N, kRankUnknown);
    std::vector<uint32_t> num(n_below, 0), stack, stack_parent;
    size_t b, e;
    children(0, &b, &e);
    for (size_t j = e; j-- > b;) {
        stack.push_back(by_parent[j]);
        stack_parent.push_back(0);
    }
    uint32_t at = 1;
    while (!stack.empty()) {
        const uint32_t k = stack.back(), pn = stack_parent.back();
        stack.pop_back();
        stack_parent.pop_back();
        if (at >= N) throw std::runtime_error("internal: the device tree numbers more nodes than it has");
        const uint32_t me = at++;
        num[k] = me;
        T.parent[me] = pn;
        T.tax[me] = all[k];
        T.rank[me] = rk[k];
        T.depth[me] = T.depth[pn] + 1;
        T.max_depth = std::max(T.max_depth, T.depth[me]);
        children(all[k], &b, &e);
        for (size_t j = e; j-- > b;) {
            stack.push_back(by_parent[j]);
            stack_parent.push_back(me);
        }
    }
    if (at != N) throw std::runtime_error("internal: " + std::to_string(N - at) + " nodes of the device tree hang under no root");
    for (size_t i = 0; i < N; i++) T.last[i] = (uint32_t)i;
    for (size_t i = N; i-- > 1;) T.last[T.parent[i]] = std::max(T.last[T.parent[i]], T.last[i]);
    // ---- the union's nodes ----
    T.u_tax = taxa;
    T.u_node.resize(taxa.size());
    for (size_t j = 0; j < taxa.size(); j++)
        T.u_node[j] = taxa[j] ? num[(size_t)(std::lower_bound(all.begin(), all.end(), taxa[j]) - all.begin())] : 0;
    return T;
}

LcaState::LcaState(int device_, hipStream_t stream_) : device(device_), stream(stream_) {
    timing = getenv("MTSV_LCA_TIMING") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    ev.create();
}

LcaState::~LcaState() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    if (stream) (void)hipStreamSynchronize(stream);
}

void Fold::lca(const Taxonomy& tx, uint32_t edit_slack, Fold* out, std::vector<mtsv_clade_stats>* rows, uint64_t* total_reads, float* device_ms) {
    if (out == this) throw std::runtime_error("arg: the output fold is the fold itself");
    if (out && out->device != device) throw std::runtime_error("arg: the output fold is on device " + std::to_string(out->device) + ", the fold on device " + std::to_string(device));
    if (out && out->grain != MTSV_GRAIN_TAXID) throw std::runtime_error("arg: the grain of the output fold is not MTSV_GRAIN_TAXID: a read's LCA is one (read, TaxID, edit) record");
    if (rows) rows->clear();
    if (total_reads) *total_reads = 0;
    if (device_ms) *device_ms = 0;
    if (!n) {  // (no read has a record: nothing is built or launched)
        if (out) out->reset(n_reads);
        return;
    }
    HIP_CHECK(hipSetDevice(device));
    if (!lca_state) lca_state.reset(new LcaState(device, stream));
    LcaState& L = *lca_state;
    // ---- the device tree: only when the union or the taxonomy changed ----
    const double t0 = L.timing ? now_ms() : 0;
    const bool rebuild = L.tree_serial != tx.serial || L.tree_taxa != taxa;
    if (rebuild) {
        LcaTree T = LcaTree::build(tx, taxa);
        const uint64_t N = T.nodes(), U = T.u_tax.size();
        std::vector<uint32_t> img;
        img.reserve(3 * N + 2 * U);
        for (const auto* v : {&T.parent, &T.last, &T.tax, &T.u_tax, &T.u_node}) img.insert(img.end(), v->begin(), v->end());
        L.tree_serial = 0;  // (the device's copy is being replaced)
        L.d_tree.room(stream, img.size(), "the device tree");
        HIP_CHECK(hipMemcpyAsync(L.d_tree.p, img.data(), img.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        L.tree = std::move(T);
        L.tree_taxa = taxa;
        L.tree_serial = tx.serial;
    }
    const LcaTree& T = L.tree;
    const uint32_t N = T.nodes(), U = (uint32_t)T.u_tax.size();
    const uint32_t *d_parent = L.d_tree.p, *d_last = d_parent + N, *d_tax = d_last + N, *d_u_tax = d_tax + N, *d_u_node = d_u_tax + U;
    const double t1 = L.timing ? now_ms() : 0;
    // ---- the reads with a record ----
    const uint32_t tiles = lca_tiles(n, lca_tile);
    L.d_tile_cnt.room(stream, tiles, "the tiles' heads");
    L.d_tile_off.room(stream, (uint64_t)tiles + 1, "the tiles' offsets");
    L.d_sums.room(stream, (uint64_t)std::max(scan_tiles(tiles), scan_tiles(N)) + 1, "the scans' sums");
    L.d_ctr.room(stream, kLcaCounters + 2, "the counters");
    L.d_node.room(stream, 3ull * N + 1, "the nodes' counts");
    uint64_t* d_n_slots = L.d_ctr.p + kLcaCounters;
    HIP_CHECK(hipMemsetAsync(L.d_ctr.p, 0, (kLcaCounters + 2) * sizeof(uint64_t), stream));
    HIP_CHECK(hipEventRecord(L.ev[0], stream));
    launch_lca_heads(stream, grain, d_rec[cur].p, (uint32_t)n, lca_tile, L.d_tile_cnt.p);
    launch_scan(stream, L.d_tile_cnt.p, tiles, L.d_sums.p, d_n_slots, L.d_tile_off.p);
    HIP_CHECK(hipEventRecord(L.ev[1], stream));
    uint64_t R = 0;
    HIP_CHECK(hipMemcpyAsync(&R, d_n_slots, sizeof R, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (!R || R > n) throw std::runtime_error("internal: " + std::to_string(n) + " records of " + std::to_string(R) + " reads");
    // ---- room for one record per read: the output fold's other array, a new pair when it is too small, or the call's own ----
    L.d_slot.room(stream, 3 * R, "the reads' spans");
    if (!out) L.d_out.room(stream, R * sizeof(mtsv_assignment), "the reads' records");
    Staged st = out ? out->stage_write(R, "an output fold") : Staged{};  // (an error below frees a pair it holds: the output fold stays as it was)
    uint8_t* dst = out ? st.dst : L.d_out.p;
    std::vector<uint32_t> direct(N), clade(N);
    uint64_t ctr[kLcaCounters + 2] = {};
    float ms[5] = {0, 0, 0, 0, 0};
    double t2 = 0, t3 = 0;
    uint32_t *d_m = L.d_slot.p, *d_lo = d_m + R, *d_hi = d_lo + R;
    uint32_t *d_direct = L.d_node.p, *d_prefix = d_direct + N, *d_clade = d_prefix + N + 1;
    HIP_CHECK(hipMemsetAsync(d_m, 0xff, 2 * R * sizeof(uint32_t), stream));  // (m and lo: all ones)
    HIP_CHECK(hipMemsetAsync(d_hi, 0, R * sizeof(uint32_t), stream));
    HIP_CHECK(hipMemsetAsync(d_direct, 0, (size_t)N * sizeof(uint32_t), stream));
    HIP_CHECK(hipEventRecord(L.ev[2], stream));
    launch_lca_min(stream, grain, d_rec[cur].p, (uint32_t)n, lca_tile, L.d_tile_off.p, (uint32_t)R, d_m, dst);
    HIP_CHECK(hipEventRecord(L.ev[3], stream));
    launch_lca_span(stream, grain, d_rec[cur].p, (uint32_t)n, lca_tile, L.d_tile_off.p, (uint32_t)R, d_m, edit_slack, d_u_tax, d_u_node, U, d_lo, d_hi,
                    L.d_ctr.p);
    HIP_CHECK(hipEventRecord(L.ev[4], stream));
    launch_lca_walk(stream, (uint32_t)R, N, T.max_depth, d_lo, d_hi, d_m, d_parent, d_last, d_tax, dst, d_direct, L.d_ctr.p);
    HIP_CHECK(hipEventRecord(L.ev[5], stream));
    launch_scan(stream, d_direct, N, L.d_sums.p, d_n_slots + 1, d_prefix);
    launch_lca_clade(stream, N, d_last, d_prefix, d_clade);
    HIP_CHECK(hipEventRecord(L.ev[6], stream));
    if (L.timing) HIP_CHECK(hipStreamSynchronize(stream));
    t2 = L.timing ? now_ms() : 0;
    HIP_CHECK(hipMemcpyAsync(ctr, L.d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(direct.data(), d_direct, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(clade.data(), d_clade, (size_t)N * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    t3 = L.timing ? now_ms() : 0;
    if (ctr[kLcaCtrMissing])
        throw std::runtime_error("internal: " + std::to_string(ctr[kLcaCtrMissing]) + " records of the fold carry a TaxID that is not in its union of " + std::to_string(U) + " TaxIDs");
    if (ctr[kLcaCtrWalk])
        throw std::runtime_error("internal: the walks of " + std::to_string(ctr[kLcaCtrWalk]) + " reads did not end within the " + std::to_string(T.max_depth) + " levels of the device tree");
    if (ctr[kLcaCounters + 1] != R || clade[0] != R)
        throw std::runtime_error("internal: " + std::to_string(R) + " reads, " + std::to_string(ctr[kLcaCounters + 1]) + " counted at their nodes, " + std::to_string(clade[0]) + " under the super-root");
    HIP_CHECK(hipEventElapsedTime(&ms[0], L.ev[0], L.ev[1]));
    for (int k = 1; k < 5; k++) HIP_CHECK(hipEventElapsedTime(&ms[k], L.ev[k + 1], L.ev[k + 2]));
    // ---- nothing can fail from here: the output fold takes the records, the caller the rows ----
    if (out) {
        out->commit(st, R);
        out->n_reads = n_reads;
        out->taxa.clear();
        for (uint32_t i = 0; i < N; i++)
            if (direct[i]) out->taxa.push_back(T.tax[i]);
        std::sort(out->taxa.begin(), out->taxa.end());
    }
    if (rows)
        for (uint32_t i = 0; i < N; i++)
            if (clade[i]) rows->push_back(mtsv_clade_stats{T.tax[i], T.tax[T.parent[i]], T.rank[i], T.depth[i], direct[i], clade[i]});
    if (total_reads) *total_reads = R;
    const float all_ms = ms[0] + ms[1] + ms[2] + ms[3] + ms[4];
    if (device_ms) *device_ms = all_ms;
    if (trace)
        fprintf(stderr, "[lca] %llu records of %llu reads over %u nodes (%u TaxIDs, depth %u) in %u tiles of %u, slack %u: %.3f ms\n", (unsigned long long)n,
                (unsigned long long)R, N, U, T.max_depth, tiles, lca_tile, edit_slack, all_ms);
    // MTSV_LCA_TIMING=1: where a call spends its time (tools/lca_ab.py reads this line)
    if (L.timing)
        fprintf(stderr, "[lca timing] records %llu reads %llu nodes %u taxa %u rebuilt %d; tree %.3f ms, heads %.3f ms, min %.3f ms, span %.3f ms, walk %.3f ms, "
                        "clade %.3f ms, download %.3f ms, call %.3f ms\n",
                (unsigned long long)n, (unsigned long long)R, N, U, rebuild ? 1 : 0, t1 - t0, ms[0], ms[1], ms[2], ms[3], ms[4], t3 - t2, now_ms() - t0);
}

}  // namespace mtsv
