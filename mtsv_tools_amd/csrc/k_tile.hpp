// k_tile.hpp -- the tile scaffold of the record kernels k_pair.hip and k_abund.hip, and the block-wide sum that the other
// tiled passes (k_fold.hip, k_parse.hip, k_text.hip, k_compact.hip, k_pile.hip) share with it.  Device code only.
// (k_lca.hip, where the shape was first written, keeps its own text of it: on this header k_lca_span measured 0.002 ms of
// 0.264 slower than before, outside the run-to-run spread -- profiles/README.md, r33.  It follows the same rules.)
//
// A sorted list of n records is cut into SEGMENTS of consecutive records with one key (a read; a run of one (read, tax_id)).
// The first record of a segment is its HEAD, and the heads before a record, counted over the list, number its segment (its
// SLOT).  The kernels are record-parallel: a workgroup of THREADS lanes per TILE of `tile` records, a STRETCH of
// max(tile / THREADS, 1) consecutive records per lane; no lane walks a segment, so a read of thousands of records costs what
// thousands of reads of one record do.  Three launches use the scaffold:
//   heads   tile_lane marks the heads of the lane's stretch as bits of a word; block_excl_sum of the lanes' counts gives the
//           heads of the tile before the stretch and in the tile.  The tile's count goes out; launch_scan over the tiles'
//           counts gives `base`, the heads before the tile.
//   reduce  a record's RANK among the tile's heads (tile_rank) is 0 for the records in front of the tile's first head and r
//           for those of the tile's r-th segment: rank r is slot base + r - 1.  Every record goes into the LDS cell of its rank
//           (seg_lds_reduce): a wavefront whose records all share the rank reduces by shuffles and sends one lane.
//   flush   tile_flush hands every rank's cell to its slot.  A segment that lies wholly inside the tile is this tile's alone:
//           INTERIOR SEGMENTS STORE.  Only the tile's first segment (rank 0: it began in an earlier tile) and its last (when
//           the record behind the tile is no head, it goes on in the next) can be shared with a neighbour: EDGE SEGMENTS USE AN
//           ATOMIC, into a cell that the host set to the reduction's identity.  A tile without a head has rank 0 alone, first
//           and last at once.  So no global address takes more than two atomics per tile, whatever the segments' lengths, and
//           a stored slot is written by exactly one tile.
// What a head is comes from the kernel file as a functor H:
//   H::key(i)           the key of record i, loaded once
//   H::head(prev, cur)  from the keys of a record's predecessor and the record: bit 0 set when it is a head, bit 1 when it is a
//                       head of the SECOND KIND (k_abund.hip counts read heads and run heads in one pass)
// Record 0 is a head of every kind.
#pragma once
#include "kernels_common.hpp"

namespace mtsv {
namespace {

// the sum of v over this lane and the lanes of its wavefront below it
__device__ inline uint32_t wave_incl_sum(uint32_t v) {
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, d);
        if ((int)lane_id() >= d) v += up;
    }
    return v;
}

struct BlockSum {
    uint32_t before, total;  // the sum over the lanes below this one; over the workgroup
};

// The block-wide exclusive sum of one number per lane.  wsum: THREADS / 64 u32 of LDS.  Holds exactly one __syncthreads(),
// between the wavefronts' sums going to wsum and their being read: what a caller wrote to LDS before the call is visible to
// the workgroup after it, and callers rely on that.  (Two sums packed into one word are summed at once when neither can carry
// into the other: k_abund.hip.)
template <uint32_t THREADS>
__device__ inline BlockSum block_excl_sum(uint32_t mine, uint32_t* wsum) {
    const uint32_t incl = wave_incl_sum(mine), wave = threadIdx.x / kWave;
    if (lane_id() == (uint32_t)kWave - 1) wsum[wave] = incl;
    __syncthreads();
    BlockSum s{incl - mine, 0};
    for (uint32_t w = 0; w < THREADS / kWave; w++) {
        const uint32_t x = wsum[w];
        if (w < wave) s.before += x;
        s.total += x;
    }
    return s;
}

// What a lane knows of its tile: its stretch of positions [p0, p1), which of them are heads (bit k: position p0 + k), the heads
// of the tile before p0, the heads of the tile.  heads2, before2, total2: the same of the second kind, 0 when one is counted
// (KINDS = 1).
template <uint32_t KINDS>
struct TileLane {
    uint64_t i0;  // the tile's first record
    uint32_t nt;  // its records
    uint32_t ipt, p0, p1;
    uint32_t heads, before, total;
    uint32_t heads2, before2, total2;
};

// the head bits of record i < n
template <class H>
__device__ inline uint32_t tile_heads_at(const H& h, uint64_t i) {
    return i ? h.head(h.key(i - 1), h.key(i)) : 3u;
}

// wsum: THREADS / 64 u32 of LDS; holds block_excl_sum's __syncthreads().  A lane loads each record of its stretch once and the
// predecessor of its first record once.  KINDS = 2 counts the second kind as well, both counts in one word: a tile of up to
// 65535 records.  A stretch is at most 32 records (the callers assert it of their largest tile).
template <uint32_t THREADS, uint32_t KINDS = 1, class H>
__device__ inline TileLane<KINDS> tile_lane(uint32_t n, uint32_t tile, uint32_t* wsum, const H& h) {
    static_assert(KINDS == 1 || KINDS == 2, "heads of one kind, or of two");
    TileLane<KINDS> t;
    t.i0 = (uint64_t)blockIdx.x * tile;
    t.nt = (uint32_t)min((uint64_t)tile, (uint64_t)n - t.i0);
    // (every tile these kernels accept is a power of two, so this is the ceiling of tile / THREADS that k_fold and k_text use)
    t.ipt = max(tile / THREADS, 1u);
    t.p0 = min(threadIdx.x * t.ipt, t.nt);
    t.p1 = min(t.p0 + t.ipt, t.nt);
    t.heads = t.heads2 = 0;
    if (t.p0 < t.p1) {
        const uint64_t first = t.i0 + t.p0;
        auto prev = first ? h.key(first - 1) : decltype(h.key(0)){};
        for (uint32_t p = t.p0; p < t.p1; p++) {
            const auto cur = h.key(t.i0 + p);
            const uint32_t bits = h.head(prev, cur);
            if (t.i0 + p == 0 || (bits & 1)) t.heads |= 1u << (p - t.p0);
            if (KINDS == 2 && (t.i0 + p == 0 || (bits & 2))) t.heads2 |= 1u << (p - t.p0);
            prev = cur;
        }
    }
    const uint32_t mine = KINDS == 2 ? (uint32_t)__popc(t.heads) << 16 | (uint32_t)__popc(t.heads2) : (uint32_t)__popc(t.heads);
    const BlockSum s = block_excl_sum<THREADS>(mine, wsum);
    t.before = KINDS == 2 ? s.before >> 16 : s.before;
    t.total = KINDS == 2 ? s.total >> 16 : s.total;
    t.before2 = KINDS == 2 ? s.before & 0xffffu : 0;
    t.total2 = KINDS == 2 ? s.total & 0xffffu : 0;
    return t;
}

// the rank of position p0 + k among the tile's heads: 0 for the records in front of the tile's first head
__device__ inline uint32_t tile_rank(uint32_t heads, uint32_t before, uint32_t k) { return before + (uint32_t)__popc(heads & (0xffffffffu >> (31 - k))); }

// cell[r] = min (MAX: max) of cell[r] and v for the lanes with act set.  Called by every lane of the wavefront together.  When
// all its active lanes share r -- a segment of thousands of records -- the wavefront reduces by shuffles and one lane goes to LDS.
template <bool MAX>
__device__ inline void seg_lds_reduce(uint32_t* cell, bool act, uint32_t r, uint32_t v) {
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

// The flush: f(slot, r, shared) for every rank r of the tile that has records and a slot below n_slots, the workgroup's lanes
// striding the ranks; call it behind the __syncthreads() that ends the reduce.  shared: a neighbouring tile may hold records of
// the segment, so the cell goes out with an atomic; otherwise f stores.  KIND = 1: the ranks, base and slots of the second kind.
//   rank 0 has records when the tile's first record is no head; then the segment began in an earlier tile and base >= 1.  (A
//     test on the cell's value cannot say so: a cell may hold the identity with records in it.)
//   rank total, the tile's last segment, goes on when the record behind the tile is no head.
template <uint32_t THREADS, uint32_t KIND = 0, uint32_t KINDS, class H, class F>
__device__ inline void tile_flush(const TileLane<KINDS>& t, uint32_t n, uint32_t base, uint64_t n_slots, const H& h, F f) {
    static_assert(KIND < KINDS, "the lane counted no heads of this kind");
    const uint32_t total = KIND ? t.total2 : t.total;
    const uint64_t next = t.i0 + t.nt;
    const bool open = base > 0 && !(tile_heads_at(h, t.i0) >> KIND & 1);
    const bool goes_on = next < n && !(tile_heads_at(h, next) >> KIND & 1);
    for (uint32_t r = threadIdx.x; r <= total; r += THREADS) {
        if (r == 0 && !open) continue;
        const uint64_t slot = (uint64_t)base + r - 1;
        if (slot >= n_slots) continue;
        f(slot, r, r == 0 || (r == total && goes_on));
    }
}

}  // namespace
}  // namespace mtsv
