// k_lca.hip -- per read of a sorted list of assignment records the lowest common ancestor of its best taxa, and the reads per
// clade (lca.hip, mtsv_fold_lca).
//
// The tree comes numbered in PREORDER (lca.hip builds it from the fold's TaxIDs and their ancestors): node 0 is the super-root,
// parent[i] < i, and the subtree of i is the interval [i, last[i]].  So a is an ancestor-or-self of b exactly when
// a <= b <= last[a], and the LCA of a set is found from its smallest and largest member alone: walk up from the smallest until
// the interval holds the largest.  Per read that is a segmented min and max of node numbers and one walk; per clade the
// difference of two prefix sums of the per-node counts.  Nothing is propagated through the tree.
//
// Record-parallel, a workgroup per tile of `tile` records, a stretch of tile / 256 consecutive records per lane; no lane walks a
// read's records.  A HEAD is a record whose read differs from its predecessor's (a 64-bit compare); the heads before a record,
// counted over the list, number its read (its SLOT):
//   k_lca_heads  tile_cnt[t] = the heads of tile t                            (then launch_scan: tile_off, and the slots in all)
//   k_lca_min    the segmented minimum of edit: every record does an LDS atomicMin into the cell of its rank among the tile's
//                heads -- a wavefront whose records all share the rank reduces by shuffles and sends one lane.  A segment that
//                lies wholly inside the tile is stored to m[slot]; only the tile's first segment (it began in an earlier tile)
//                and its last (it goes on in the next) can be shared with a neighbour, and those go out with one atomicMin
//                each.  Heads write out[slot].read.
//   k_lca_span   a launch of its own: m must be complete across tiles before a record is filtered.  A record with
//                edit <= m[slot] + slack (saturating) finds its node by binary search in the union's TaxIDs; min and max of the
//                node numbers by the same rule as above: interior segments store, the at most two edge segments use
//                atomicMin / atomicMax.  A TaxID that is not in the table is counted apart (the host makes an error of it).
//   k_lca_walk   a lane per read: from lo up the parents until last[a] >= hi, at most max_depth steps -- a walk that has not
//                ended by then is counted and writes nothing; it never spins.  Writes (read, tax[a], m) and adds the read to
//                direct[a]: the lanes of a wavefront that hold the same node go in as one add.
//   (launch_scan over direct)
//   k_lca_clade  a lane per node: clade[i] = prefix[last[i] + 1] - prefix[i]
// No global address takes more than two atomics per tile in k_lca_min and k_lca_span, whatever the lengths of the reads.
#include <hip/hip_runtime.h>

#include <string>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kLcaThreads = 256;
constexpr uint32_t kLcaWaves = kLcaThreads / kWave;
constexpr uint32_t kLcaStretchMax = kLcaTileMax / kLcaThreads;  // records per lane at the largest tile
static_assert(kLcaStretchMax <= 32, "the heads of a lane's stretch are kept as bits of one word");

// What a lane knows of its tile: its stretch of positions [p0, p1), which of them are heads (bit k: position p0 + k), the heads
// of the tile before p0, the heads of the tile
struct LcaLane {
    uint64_t i0;  // the tile's first record
    uint32_t nt;  // its records
    uint32_t ipt, p0, p1, heads, before, total;
};

// wsum: kLcaWaves u32 of LDS.  Holds a __syncthreads(): what the caller wrote to LDS before the call is visible after it.
template <uint32_t W>
__device__ inline LcaLane lca_lane(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, uint32_t* wsum) {
    LcaLane t;
    t.i0 = (uint64_t)blockIdx.x * tile;
    t.nt = (uint32_t)min((uint64_t)tile, (uint64_t)n - t.i0);
    t.ipt = max(tile / kLcaThreads, 1u);
    t.p0 = min(threadIdx.x * t.ipt, t.nt);
    t.p1 = min(t.p0 + t.ipt, t.nt);
    t.heads = 0;
    if (t.p0 < t.p1) {
        const uint64_t first = t.i0 + t.p0;
        uint64_t prev = first ? rec_read_of<W>(rec, first - 1) : 0;
        for (uint32_t p = t.p0; p < t.p1; p++) {
            const uint64_t read = rec_read_of<W>(rec, t.i0 + p);
            if (t.i0 + p == 0 || read != prev) t.heads |= 1u << (p - t.p0);
            prev = read;
        }
    }
    const uint32_t mine = (uint32_t)__popc(t.heads);
    uint32_t incl = mine;
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if ((int)lane_id() >= d) incl += up;
    }
    const uint32_t wave = threadIdx.x / kWave;
    if (lane_id() == (uint32_t)kWave - 1) wsum[wave] = incl;
    __syncthreads();
    t.before = incl - mine;
    t.total = 0;
    for (uint32_t w = 0; w < kLcaWaves; w++) {
        const uint32_t s = wsum[w];
        if (w < wave) t.before += s;
        t.total += s;
    }
    return t;
}

// the rank of position p0 + k among the tile's heads: 0 for the records in front of the tile's first head
__device__ inline uint32_t lca_rank(const LcaLane& t, uint32_t k) { return t.before + (uint32_t)__popc(t.heads & (0xffffffffu >> (31 - k))); }

// cell[r] = min (MAX: max) of cell[r] and v for the lanes with act set.  Called by every lane of the wavefront together.  When
// all its active lanes share r -- a read of thousands of records -- the wavefront reduces by shuffles and one lane goes to LDS.
template <bool MAX>
__device__ inline void lca_lds_reduce(uint32_t* cell, bool act, uint32_t r, uint32_t v) {
    const unsigned long long am = __ballot(act);
    if (!am) return;
    const uint32_t leader = (uint32_t)__builtin_ctzll(am);
    const uint32_t r0 = (uint32_t)__shfl((int)r, (int)leader);
    const unsigned long long same = __ballot(act && r == r0);
    if (same == am && __popcll(am) > 1) {
        uint32_t x = act ? v : (MAX ? 0u : 0xffffffffu);
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const uint32_t y = (uint32_t)__shfl_xor((int)x, d);
            x = MAX ? max(x, y) : min(x, y);
        }
        if (lane_id() == leader) {
            if (MAX) atomicMax(&cell[r0], x);
            else atomicMin(&cell[r0], x);
        }
    } else if (act) {
        if (MAX) atomicMax(&cell[r], v);
        else atomicMin(&cell[r], v);
    }
}

// the tile's last record and the one behind it are of one read: the tile's last segment goes on in the next tile
template <uint32_t W>
__device__ inline bool lca_goes_on(const uint32_t* __restrict__ rec, uint32_t n, const LcaLane& t) {
    const uint64_t next = t.i0 + t.nt;
    return next < n && rec_read_of<W>(rec, next) == rec_read_of<W>(rec, next - 1);
}

template <uint32_t W>
__global__ __launch_bounds__(kLcaThreads) void k_lca_heads(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t wsum[kLcaWaves];
    const LcaLane t = lca_lane<W>(rec, n, tile, wsum);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = t.total;
}

template <uint32_t W>
__global__ __launch_bounds__(kLcaThreads) void k_lca_min(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, const uint32_t* __restrict__ tile_off,
                                                        uint32_t n_slots, uint32_t* __restrict__ m, uint32_t* __restrict__ out) {
    __shared__ uint32_t wsum[kLcaWaves];
    __shared__ uint32_t smin[kLcaTileMax + 1];  // by rank among the tile's heads
    for (uint32_t r = threadIdx.x; r <= tile; r += kLcaThreads) smin[r] = 0xffffffffu;
    const LcaLane t = lca_lane<W>(rec, n, tile, wsum);
    const uint32_t base = tile_off[blockIdx.x];  // the heads before the tile: rank r is slot base + r - 1
    for (uint32_t k = 0; k < t.ipt; k++) {       // (ipt is the same in every lane)
        const bool act = t.p0 + k < t.p1;
        uint32_t r = 0, e = 0;
        if (act) {
            const uint64_t i = t.i0 + t.p0 + k;
            r = lca_rank(t, k);
            e = rec[i * W + W - 1];
            if (t.heads >> k & 1) {
                const uint64_t slot = (uint64_t)base + r - 1;
                if (slot < n_slots) *reinterpret_cast<uint2*>(out + slot * 4) = *reinterpret_cast<const uint2*>(rec + i * W);
            }
        }
        lca_lds_reduce<false>(smin, act, r, e);
    }
    __syncthreads();
    // the segments: rank 0 is there when the tile's first record is no head -- it began in an earlier tile
    for (uint32_t r = threadIdx.x; r <= t.total; r += kLcaThreads) {
        const uint32_t v = smin[r];
        if (r == 0 && (v == 0xffffffffu || base == 0)) continue;  // (no record in front of the first head; v is all ones then)
        const uint64_t slot = (uint64_t)base + r - 1;
        if (slot >= n_slots) continue;
        if (r == 0 || (r == t.total && lca_goes_on<W>(rec, n, t))) atomicMin(&m[slot], v);
        else m[slot] = v;
    }
}

template <uint32_t W>
__global__ __launch_bounds__(kLcaThreads) void k_lca_span(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, const uint32_t* __restrict__ tile_off,
                                                         uint32_t n_slots, const uint32_t* __restrict__ m, uint32_t slack,
                                                         const uint32_t* __restrict__ u_tax, const uint32_t* __restrict__ u_node, uint32_t n_union,
                                                         uint32_t* __restrict__ lo, uint32_t* __restrict__ hi, unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t wsum[kLcaWaves];
    __shared__ uint32_t smin[kLcaTileMax + 1], smax[kLcaTileMax + 1];
    for (uint32_t r = threadIdx.x; r <= tile; r += kLcaThreads) {
        smin[r] = 0xffffffffu;
        smax[r] = 0;
    }
    const LcaLane t = lca_lane<W>(rec, n, tile, wsum);
    const uint32_t base = tile_off[blockIdx.x];
    uint32_t n_missing = 0;
    for (uint32_t k = 0; k < t.ipt; k++) {
        bool act = t.p0 + k < t.p1;
        uint32_t r = 0, node = 0;
        if (act) {
            const uint64_t i = t.i0 + t.p0 + k;
            r = lca_rank(t, k);
            const uint64_t slot = (uint64_t)base + r - 1;  // (a list begins with a head: base + r >= 1)
            act = slot < n_slots;
            if (act) {
                const uint32_t best = m[slot];
                const uint32_t bound = best > 0xffffffffu - slack ? 0xffffffffu : best + slack;
                act = rec[i * W + W - 1] <= bound;
            }
            if (act) {
                const uint32_t j = find_u32(u_tax, n_union, rec[i * W + 2]);
                if (j < n_union) node = u_node[j];
                else {
                    n_missing++;
                    act = false;
                }
            }
        }
        lca_lds_reduce<false>(smin, act, r, node);
        lca_lds_reduce<true>(smax, act, r, node);
    }
    if (n_missing) atomicAdd(&ctr[kLcaCtrMissing], (unsigned long long)n_missing);
    __syncthreads();
    for (uint32_t r = threadIdx.x; r <= t.total; r += kLcaThreads) {
        const uint32_t a = smin[r], b = smax[r];
        if (a == 0xffffffffu) continue;  // (no record of the segment entered here: none in front of the first head, or none within the bound)
        if (r == 0 && base == 0) continue;
        const uint64_t slot = (uint64_t)base + r - 1;
        if (slot >= n_slots) continue;
        if (r == 0 || (r == t.total && lca_goes_on<W>(rec, n, t))) {
            atomicMin(&lo[slot], a);
            atomicMax(&hi[slot], b);
        } else {
            lo[slot] = a;
            hi[slot] = b;
        }
    }
}

__global__ __launch_bounds__(kLcaThreads) void k_lca_walk(uint32_t n_slots, uint32_t n_nodes, uint32_t max_depth, const uint32_t* __restrict__ lo,
                                                         const uint32_t* __restrict__ hi, const uint32_t* __restrict__ m,
                                                         const uint32_t* __restrict__ parent, const uint32_t* __restrict__ last,
                                                         const uint32_t* __restrict__ tax, uint32_t* __restrict__ out, uint32_t* __restrict__ direct,
                                                         unsigned long long* __restrict__ ctr) {
    const uint64_t s = (uint64_t)blockIdx.x * kLcaThreads + threadIdx.x;
    bool ok = false, bad = false;
    uint32_t a = 0;
    if (s < n_slots) {
        a = lo[s];
        const uint32_t b = hi[s];
        if (a > b || b >= n_nodes) {
            bad = true;
        } else {
            // (a node at depth d reaches the super-root, whose interval is the whole tree, in d steps)
            for (uint32_t step = 0; step < max_depth && last[a] < b; step++) {
                a = parent[a];
                if (a >= n_nodes) break;
            }
            ok = a < n_nodes && a <= b && last[a] >= b;
            bad = !ok;
        }
        if (ok) *reinterpret_cast<uint2*>(out + s * 4 + 2) = make_uint2(tax[a], m[s]);
    }
    // the reads of the wavefront to their nodes, node by node: the lanes that hold the node of the first lane still waiting add
    // their number at once
    unsigned long long todo = __ballot(ok);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t node = (uint32_t)__shfl((int)a, (int)leader);
        const unsigned long long same = __ballot(ok && a == node);
        if (lane_id() == leader) atomicAdd(&direct[node], (uint32_t)__popcll(same));
        todo &= ~same;
    }
    const unsigned long long bm = __ballot(bad);
    if (bm && lane_id() == 0) atomicAdd(&ctr[kLcaCtrWalk], (unsigned long long)__popcll(bm));
}

__global__ __launch_bounds__(kLcaThreads) void k_lca_clade(uint32_t n_nodes, const uint32_t* __restrict__ last, const uint32_t* __restrict__ prefix,
                                                          uint32_t* __restrict__ clade) {
    const uint64_t i = (uint64_t)blockIdx.x * kLcaThreads + threadIdx.x;
    if (i >= n_nodes) return;
    const uint32_t l = last[i];
    clade[i] = l < n_nodes && l >= i ? prefix[l + 1] - prefix[i] : 0;
}

void lca_check(int grain, uint32_t tile) {
    if (grain != kCollapseGrainTaxid && grain != kCollapseGrainTaxidGi && grain != kCollapseGrainLong)
        throw std::runtime_error("internal: lca at grain " + std::to_string(grain));
    if (tile < 64 || tile > kLcaTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: lca tile of " + std::to_string(tile) + " records");
}

}  // namespace

uint32_t lca_tiles(uint64_t n, uint32_t tile) { return cdiv(n, tile); }

void launch_lca_heads(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, uint32_t* tile_cnt) {
    lca_check(grain, tile);
    const uint32_t tiles = lca_tiles(n, tile);
    if (!tiles) return;
    if (grain == kCollapseGrainTaxid) hipLaunchKernelGGL(k_lca_heads<4>, dim3(tiles), dim3(kLcaThreads), 0, s, (const uint32_t*)rec, n, tile, tile_cnt);
    else hipLaunchKernelGGL(k_lca_heads<6>, dim3(tiles), dim3(kLcaThreads), 0, s, (const uint32_t*)rec, n, tile, tile_cnt);
}

void launch_lca_min(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, const uint32_t* tile_off, uint32_t n_slots, uint32_t* m,
                    void* out) {
    lca_check(grain, tile);
    const uint32_t tiles = lca_tiles(n, tile);
    if (!tiles || !n_slots) return;
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL(k_lca_min<4>, dim3(tiles), dim3(kLcaThreads), 0, s, (const uint32_t*)rec, n, tile, tile_off, n_slots, m, (uint32_t*)out);
    else
        hipLaunchKernelGGL(k_lca_min<6>, dim3(tiles), dim3(kLcaThreads), 0, s, (const uint32_t*)rec, n, tile, tile_off, n_slots, m, (uint32_t*)out);
}

void launch_lca_span(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, const uint32_t* tile_off, uint32_t n_slots,
                     const uint32_t* m, uint32_t slack, const uint32_t* u_tax, const uint32_t* u_node, uint32_t n_union, uint32_t* lo, uint32_t* hi,
                     uint64_t* ctr) {
    lca_check(grain, tile);
    const uint32_t tiles = lca_tiles(n, tile);
    if (!tiles || !n_slots) return;
    auto* c = reinterpret_cast<unsigned long long*>(ctr);
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL(k_lca_span<4>, dim3(tiles), dim3(kLcaThreads), 0, s, (const uint32_t*)rec, n, tile, tile_off, n_slots, m, slack, u_tax, u_node,
                           n_union, lo, hi, c);
    else
        hipLaunchKernelGGL(k_lca_span<6>, dim3(tiles), dim3(kLcaThreads), 0, s, (const uint32_t*)rec, n, tile, tile_off, n_slots, m, slack, u_tax, u_node,
                           n_union, lo, hi, c);
}

void launch_lca_walk(hipStream_t s, uint32_t n_slots, uint32_t n_nodes, uint32_t max_depth, const uint32_t* lo, const uint32_t* hi, const uint32_t* m,
                     const uint32_t* parent, const uint32_t* last, const uint32_t* tax, void* out, uint32_t* direct, uint64_t* ctr) {
    if (!n_slots || !n_nodes) return;
    hipLaunchKernelGGL(k_lca_walk, dim3(cdiv(n_slots, kLcaThreads)), dim3(kLcaThreads), 0, s, n_slots, n_nodes, max_depth, lo, hi, m, parent, last, tax,
                       (uint32_t*)out, direct, reinterpret_cast<unsigned long long*>(ctr));
}

void launch_lca_clade(hipStream_t s, uint32_t n_nodes, const uint32_t* last, const uint32_t* prefix, uint32_t* clade) {
    if (!n_nodes) return;
    hipLaunchKernelGGL(k_lca_clade, dim3(cdiv(n_nodes, kLcaThreads)), dim3(kLcaThreads), 0, s, n_nodes, last, prefix, clade);
}

}  // namespace mtsv
