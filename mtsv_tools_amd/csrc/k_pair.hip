// k_pair.hip -- the two mates of a read pair joined into one list of (pair, tax_id, edit) records (pair.hip, mtsv_fold_pair).
//
// The list is a fold's: n records of 4 or 6 words ordered by (read, tax_id[, gi, offset]), reads 2p and 2p + 1 the mates of
// pair p.  A RUN is the records of one (read, tax_id): the segment of the tile scaffold of k_tile.hpp, where HEAD, SLOT and
// the rule of what a tile stores and what it sends with an atomic are described.  NONE is all ones: edits are below 2^31
// (counted here, refused by the host), so no sum of two reaches it.
//   k_pair_bounds  a lane per read r in 0 .. 2P: off[r] = the first record with read >= r (a lower bound on the read field)
//   k_pair_join    a lane per record.  It finds its WINDOW in the other mate's stretch [off[r ^ 1], off[(r ^ 1) + 1]) by binary
//                  searches: BOTH / EITHER the records with its tax_id (only heads search; a head of mate 1 only in EITHER,
//                  and only for whether there is one), PROPER the records with its (tax_id, gi) whose offset lies within
//                  max_insert of its own, the window clamped to [0, 2^32 - 1] (only mate 0 searches).  A window of up to
//                  lane_max records is walked for its smallest edit; a longer one puts the record on a work list, a
//                  wavefront's lanes appended with one atomic.
//                    val[i]   PROPER: edit + the window's minimum, or NONE; BOTH / EITHER: edit
//                    add[i]   (heads) what the run's minimum of val is raised by: PROPER 0; BOTH the window's minimum, or
//                             NONE; EITHER the same, `unpaired` for a run the other mate has no record for, NONE for a run
//                             of mate 1 that mate 0 shares (it is mate 0's to write)
//   k_pair_wave    a wavefront per entry of the work list, in a grid that strides it: the lanes stride the window, the
//                  minimum comes by shuffles, lane 0 stores val[i] (PROPER) or add[i]
//   k_pair_heads   tile_cnt[t] = the heads of tile t                                          (then launch_scan: tile_off)
//   k_pair_min     m[slot] = the segmented minimum of val by run; a cell that holds NONE sends no atomic.  Heads write
//                  (read, tax_id, add) of their slot.
//   k_pair_flags   a lane per slot: its value m + add, or NONE; flag_a: a run of mate 0 with a value, flag_b: one of mate 1
//                  (EITHER: the taxa only mate 1 hit)                            (then launch_scan over each: pos_a, pos_b)
//   k_pair_write   a lane per slot: (read >> 1, tax_id, value) to its place in list A or list B.  Both are ordered by
//                  (pair, tax_id) and share no key: k_fold merges them (EITHER); in the other modes A is the output.
//   k_pair_stats   per pair: both mates / exactly one mate have a record; per output record: heads by pair.  A grid of at most
//                  1024 workgroups strides both, counts in registers and adds three sums a workgroup
// No lane walks a read's records: a lane does binary searches and at most lane_max steps.
#include <hip/hip_runtime.h>

#include <string>

#include "k_tile.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kPairThreads = 256;
constexpr uint32_t kPairWaves = kPairThreads / kWave;
constexpr uint32_t kPairNone = 0xffffffffu;
constexpr uint32_t kPairStretchMax = kPairTileMax / kPairThreads;
static_assert(kPairStretchMax <= 32, "the heads of a lane's stretch are kept as bits of one word");

template <uint32_t W>
__device__ inline uint32_t pair_edit_of(const uint32_t* __restrict__ rec, uint64_t i) {
    return rec[i * W + W - 1];
}

// a segment is a run: a record is a head when its (read, tax_id) differs from its predecessor's
struct PairKey {
    uint64_t read;
    uint32_t tax;
};
template <uint32_t W>
struct PairHead {
    const uint32_t* __restrict__ rec;
    __device__ PairKey key(uint64_t i) const { return PairKey{rec_read_of<W>(rec, i), rec[i * W + 2]}; }
    __device__ static uint32_t head(const PairKey& prev, const PairKey& cur) { return prev.read != cur.read || prev.tax != cur.tax; }
};
// record i begins a run
template <uint32_t W>
__device__ inline bool pair_is_head(const uint32_t* __restrict__ rec, uint64_t i) {
    return tile_heads_at(PairHead<W>{rec}, i) & 1;
}

// the first record of [b, e) whose tax_id is not below t (UPPER: is above t)
template <uint32_t W, bool UPPER>
__device__ inline uint32_t pair_bound_tax(const uint32_t* __restrict__ rec, uint32_t b, uint32_t e, uint32_t t) {
    uint32_t lo = b, hi = e;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t x = rec[(uint64_t)mid * W + 2];
        if (UPPER ? x <= t : x < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the first record of [b, e) whose (tax_id, gi, offset) is not below (tg, o) (UPPER: is above it); 6-word records
template <bool UPPER>
__device__ inline uint32_t pair_bound_site(const uint32_t* __restrict__ rec, uint32_t b, uint32_t e, uint64_t tg, uint32_t o) {
    uint32_t lo = b, hi = e;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t* r = rec + (uint64_t)mid * 6;
        const uint64_t x = (uint64_t)r[2] << 32 | r[3];
        const bool below = x != tg ? x < tg : (UPPER ? r[4] <= o : r[4] < o);
        if (below) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the window of record i (of read `read` < n_reads) in the other mate's stretch
template <uint32_t W, bool PROPER>
__device__ inline void pair_window(const uint32_t* __restrict__ rec, const uint32_t* __restrict__ off, uint64_t i, uint64_t read, uint32_t max_insert,
                                   uint32_t* lo, uint32_t* hi) {
    const uint64_t other = read ^ 1;
    const uint32_t b = off[other], e = off[other + 1];
    if (PROPER) {
        const uint32_t* r = rec + i * W;
        const uint64_t tg = (uint64_t)r[2] << 32 | r[3];
        const uint32_t o = r[4];
        const uint32_t o_lo = o < max_insert ? 0u : o - max_insert;
        const uint32_t o_hi = o > 0xffffffffu - max_insert ? 0xffffffffu : o + max_insert;
        *lo = pair_bound_site<false>(rec, b, e, tg, o_lo);
        *hi = pair_bound_site<true>(rec, *lo, e, tg, o_hi);
    } else {
        const uint32_t t = rec[i * W + 2];
        *lo = pair_bound_tax<W, false>(rec, b, e, t);
        *hi = pair_bound_tax<W, true>(rec, *lo, e, t);
    }
}

template <uint32_t W>
__global__ __launch_bounds__(kPairThreads) void k_pair_bounds(const uint32_t* __restrict__ rec, uint32_t n, uint64_t n_reads, uint32_t* __restrict__ off) {
    const uint64_t r = (uint64_t)blockIdx.x * kPairThreads + threadIdx.x;
    if (r > n_reads) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (rec_read_of<W>(rec, mid) < r) lo = mid + 1;
        else hi = mid;
    }
    off[r] = lo;
}

template <uint32_t W, int MODE>
__global__ __launch_bounds__(kPairThreads) void k_pair_join(const uint32_t* __restrict__ rec, uint32_t n, uint64_t n_reads, const uint32_t* __restrict__ off,
                                                           uint32_t max_insert, uint32_t unpaired, uint32_t lane_max, uint32_t* __restrict__ val,
                                                           uint32_t* __restrict__ add, uint32_t* __restrict__ list, unsigned long long* __restrict__ ctr) {
    constexpr bool PROPER = MODE == kPairProper;
    const uint64_t i = (uint64_t)blockIdx.x * kPairThreads + threadIdx.x;
    bool wide = false, bad = false, beyond = false;
    if (i < n) {
        const uint64_t read = rec_read_of<W>(rec, i);
        const uint32_t edit = pair_edit_of<W>(rec, i);
        const bool head = pair_is_head<W>(rec, i);
        bad = edit >= 0x80000000u;
        beyond = read >= n_reads;
        uint32_t v = PROPER ? kPairNone : edit, a = kPairNone;
        if (!beyond) {
            const bool mate1 = read & 1;
            // who searches: PROPER every record of mate 0; BOTH the heads of mate 0; EITHER every head
            const bool search = PROPER ? !mate1 : head && (!mate1 || MODE == kPairEither);
            if (PROPER && !mate1) a = 0;
            if (search) {
                uint32_t lo, hi;
                pair_window<W, PROPER>(rec, off, i, read, max_insert, &lo, &hi);
                const uint32_t cnt = hi - lo;
                uint32_t w = kPairNone;
                if (!PROPER && mate1) {  // (EITHER: is the run mate 1's alone)
                    a = cnt ? kPairNone : unpaired;
                } else if (cnt > lane_max) {
                    wide = true;
                } else {
                    for (uint32_t j = lo; j < hi; j++) w = min(w, pair_edit_of<W>(rec, j));
                    if (PROPER) v = cnt ? edit + w : kPairNone;
                    else a = cnt ? w : MODE == kPairEither ? unpaired : kPairNone;
                }
            }
        }
        val[i] = v;
        if (head) add[i] = a;
    }
    const unsigned long long wm = __ballot(wide), bm = __ballot(bad), ym = __ballot(beyond);
    uint32_t base = 0;
    if (lane_id() == 0) {
        if (wm) base = (uint32_t)atomicAdd(&ctr[kPairCtrList], (unsigned long long)__popcll(wm));
        if (bm) atomicAdd(&ctr[kPairCtrBadEdit], (unsigned long long)__popcll(bm));
        if (ym) atomicAdd(&ctr[kPairCtrBeyond], (unsigned long long)__popcll(ym));
    }
    if (wm) {
        base = (uint32_t)__shfl((int)base, 0);
        // (every record enters at most once: base + rank < n whenever the caller zeroed the counter)
        const uint64_t at = (uint64_t)base + (uint32_t)__popcll(wm & ((1ull << lane_id()) - 1));
        if (wide && at < n) list[at] = (uint32_t)i;
    }
}

template <uint32_t W, int MODE>
__global__ __launch_bounds__(kPairThreads) void k_pair_wave(const uint32_t* __restrict__ rec, uint32_t n, uint64_t n_reads, const uint32_t* __restrict__ off,
                                                           uint32_t max_insert, const uint32_t* __restrict__ list,
                                                           const unsigned long long* __restrict__ ctr, uint32_t* __restrict__ val,
                                                           uint32_t* __restrict__ add) {
    constexpr bool PROPER = MODE == kPairProper;
    const uint64_t count = min((uint64_t)ctr[kPairCtrList], (uint64_t)n);
    const uint64_t waves = (uint64_t)gridDim.x * kPairWaves;
    for (uint64_t e = (uint64_t)blockIdx.x * kPairWaves + threadIdx.x / kWave; e < count; e += waves) {
        const uint64_t i = list[e];
        if (i >= n) continue;
        const uint64_t read = rec_read_of<W>(rec, i);
        if (read >= n_reads) continue;
        uint32_t lo, hi;
        pair_window<W, PROPER>(rec, off, i, read, max_insert, &lo, &hi);  // (the same in every lane)
        uint32_t x = kPairNone;
        for (uint64_t j = (uint64_t)lo + lane_id(); j < hi; j += kWave) x = min(x, pair_edit_of<W>(rec, j));
        for (int d = kWave / 2; d > 0; d >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, d));
        if (lane_id() == 0) {
            if (PROPER) val[i] = x == kPairNone ? kPairNone : pair_edit_of<W>(rec, i) + x;
            else add[i] = x;
        }
    }
}

template <uint32_t W>
__global__ __launch_bounds__(kPairThreads) void k_pair_heads(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t wsum[kPairWaves];
    const auto t = tile_lane<kPairThreads>(n, tile, wsum, PairHead<W>{rec});
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = t.total;
}

// m: n_slots_cap u32, all ones; slot: n_slots_cap uint4
template <uint32_t W>
__global__ __launch_bounds__(kPairThreads) void k_pair_min(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, const uint32_t* __restrict__ tile_off,
                                                          const uint32_t* __restrict__ val, const uint32_t* __restrict__ add, uint32_t n_slots_cap,
                                                          uint32_t* __restrict__ m, uint4* __restrict__ slot_rec) {
    __shared__ uint32_t wsum[kPairWaves];
    __shared__ uint32_t smin[kPairTileMax + 1];  // by rank among the tile's heads
    for (uint32_t r = threadIdx.x; r <= tile; r += kPairThreads) smin[r] = kPairNone;
    const auto t = tile_lane<kPairThreads>(n, tile, wsum, PairHead<W>{rec});
    const uint32_t base = tile_off[blockIdx.x];  // the heads before the tile: rank r is slot base + r - 1
    for (uint32_t k = 0; k < t.ipt; k++) {       // (ipt is the same in every lane)
        const bool act = t.p0 + k < t.p1;
        uint32_t r = 0, v = kPairNone;
        if (act) {
            const uint64_t i = t.i0 + t.p0 + k;
            r = tile_rank(t.heads, t.before, k);
            v = val[i];
            if (t.heads >> k & 1) {
                const uint64_t slot = (uint64_t)base + r - 1;
                if (slot < n_slots_cap) slot_rec[slot] = make_uint4(rec[i * W], rec[i * W + 1], rec[i * W + 2], add[i]);
            }
        }
        seg_lds_reduce<false>(smin, act, r, v);
    }
    __syncthreads();
    tile_flush<kPairThreads>(t, n, base, n_slots_cap, PairHead<W>{rec}, [&](uint64_t slot, uint32_t r, bool shared) {
        const uint32_t v = smin[r];
        if (!shared) m[slot] = v;
        else if (v != kPairNone) atomicMin(&m[slot], v);
    });
}

// m[s] becomes the slot's value; flag_b may be null (no list B)
__global__ __launch_bounds__(kPairThreads) void k_pair_flags(const unsigned long long* __restrict__ n_slots, uint32_t n_slots_cap,
                                                            const uint4* __restrict__ slot_rec, uint32_t* __restrict__ m, uint32_t* __restrict__ flag_a,
                                                            uint32_t* __restrict__ flag_b) {
    const uint64_t s = (uint64_t)blockIdx.x * kPairThreads + threadIdx.x;
    if (s >= n_slots_cap) return;
    uint32_t fa = 0, fb = 0;
    if (s < *n_slots) {
        const uint4 q = slot_rec[s];
        const uint32_t a = q.w, x = m[s];
        const uint32_t v = a == kPairNone || x == kPairNone ? kPairNone : x + a;
        m[s] = v;
        if (v != kPairNone) {
            if (q.x & 1) fb = 1;
            else fa = 1;
        }
    }
    flag_a[s] = fa;
    if (flag_b) flag_b[s] = fb;
}

// pos_a / pos_b: n_slots_cap + 1 entries (the scans of the flags); out_b and pos_b may be null
__global__ __launch_bounds__(kPairThreads) void k_pair_write(const unsigned long long* __restrict__ n_slots, uint32_t n_slots_cap,
                                                            const uint4* __restrict__ slot_rec, const uint32_t* __restrict__ m,
                                                            const uint32_t* __restrict__ pos_a, const uint32_t* __restrict__ pos_b, uint32_t n_a,
                                                            uint32_t n_b, uint4* __restrict__ out_a, uint4* __restrict__ out_b) {
    const uint64_t s = (uint64_t)blockIdx.x * kPairThreads + threadIdx.x;
    if (s >= n_slots_cap || s >= *n_slots) return;
    const uint4 q = slot_rec[s];
    const uint64_t pair = ((uint64_t)q.x | (uint64_t)q.y << 32) >> 1;
    const uint4 r = make_uint4((uint32_t)pair, (uint32_t)(pair >> 32), q.z, m[s]);
    const uint32_t a = pos_a[s];
    if (pos_a[s + 1] != a && a < n_a) out_a[a] = r;
    if (pos_b) {
        const uint32_t b = pos_b[s];
        if (pos_b[s + 1] != b && b < n_b) out_b[b] = r;
    }
}

__global__ __launch_bounds__(kPairThreads) void k_pair_stats(const uint32_t* __restrict__ off, uint64_t n_pairs, const uint32_t* __restrict__ out, uint32_t n_out,
                                                            unsigned long long* __restrict__ ctr) {
    // a grid that strides the pairs and the records: a lane counts in registers, a workgroup adds its sums once (one add per
    // wavefront on three addresses took two thirds of the call's device time)
    __shared__ uint32_t sums[3][kPairWaves];
    const uint64_t lanes = max(n_pairs, (uint64_t)n_out), step = (uint64_t)gridDim.x * kPairThreads;
    uint32_t cnt[3] = {0, 0, 0};  // both, one, heads
    for (uint64_t j = (uint64_t)blockIdx.x * kPairThreads + threadIdx.x; j < lanes; j += step) {
        if (j < n_pairs) {
            const uint32_t a = off[2 * j], b = off[2 * j + 1], c = off[2 * j + 2];
            cnt[0] += b > a && c > b;
            cnt[1] += (b > a) != (c > b);
        }
        if (j < n_out) cnt[2] += j == 0 || rec_read_of<4>(out, j) != rec_read_of<4>(out, j - 1);
    }
    for (int k = 0; k < 3; k++) {
        uint32_t x = cnt[k];
        for (int d = kWave / 2; d > 0; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d);
        if (lane_id() == 0) sums[k][threadIdx.x / kWave] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long x = 0;
        for (uint32_t w = 0; w < kPairWaves; w++) x += sums[threadIdx.x][w];
        if (x) atomicAdd(&ctr[kPairCtrBoth + threadIdx.x], x);
    }
}
static_assert(kPairCtrOne == kPairCtrBoth + 1 && kPairCtrJoined == kPairCtrBoth + 2, "k_pair_stats adds its three sums to consecutive counters");

void pair_check(int grain, int mode, uint32_t tile) {
    if (grain != kCollapseGrainTaxid && grain != kCollapseGrainTaxidGi && grain != kCollapseGrainLong)
        throw std::runtime_error("internal: pair at grain " + std::to_string(grain));
    if (mode != kPairBoth && mode != kPairEither && mode != kPairProper) throw std::runtime_error("internal: pair mode " + std::to_string(mode));
    if (mode == kPairProper && grain != kCollapseGrainLong) throw std::runtime_error("internal: proper pairs at grain " + std::to_string(grain));
    if (tile < 64 || tile > kPairTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: pair tile of " + std::to_string(tile) + " records");
}

}  // namespace

uint32_t pair_tiles(uint64_t n, uint32_t tile) { return cdiv(n, tile); }

void launch_pair_bounds(hipStream_t s, int grain, const void* rec, uint32_t n, uint64_t n_reads, uint32_t* off) {
    const dim3 grid(cdiv(n_reads + 1, kPairThreads)), block(kPairThreads);
    if (grain == kCollapseGrainTaxid) hipLaunchKernelGGL(k_pair_bounds<4>, grid, block, 0, s, (const uint32_t*)rec, n, n_reads, off);
    else hipLaunchKernelGGL(k_pair_bounds<6>, grid, block, 0, s, (const uint32_t*)rec, n, n_reads, off);
}

void launch_pair_join(hipStream_t s, int grain, int mode, const void* rec, uint32_t n, uint64_t n_reads, const uint32_t* off, uint32_t max_insert,
                      uint32_t unpaired, uint32_t lane_max, uint32_t* val, uint32_t* add, uint32_t* list, uint64_t* ctr) {
    pair_check(grain, mode, kPairTile);
    if (!n) return;
    const dim3 grid(cdiv(n, kPairThreads)), block(kPairThreads);
    const uint32_t* r = (const uint32_t*)rec;
    auto* c = reinterpret_cast<unsigned long long*>(ctr);
#define MTSV_PAIR_JOIN(W, M) hipLaunchKernelGGL((k_pair_join<W, M>), grid, block, 0, s, r, n, n_reads, off, max_insert, unpaired, lane_max, val, add, list, c)
    if (mode == kPairProper) MTSV_PAIR_JOIN(6, kPairProper);
    else if (grain == kCollapseGrainTaxid && mode == kPairBoth) MTSV_PAIR_JOIN(4, kPairBoth);
    else if (grain == kCollapseGrainTaxid) MTSV_PAIR_JOIN(4, kPairEither);
    else if (mode == kPairBoth) MTSV_PAIR_JOIN(6, kPairBoth);
    else MTSV_PAIR_JOIN(6, kPairEither);
#undef MTSV_PAIR_JOIN
}

void launch_pair_wave(hipStream_t s, int grain, int mode, const void* rec, uint32_t n, uint64_t n_reads, const uint32_t* off, uint32_t max_insert,
                      const uint32_t* list, const uint64_t* ctr, uint32_t* val, uint32_t* add) {
    pair_check(grain, mode, kPairTile);
    if (!n) return;
    // (the list's length stays on the device: a grid that strides it, at most eight workgroups per CU of a 256-CU device)
    const dim3 grid(std::min<uint32_t>(cdiv(n, kPairWaves), 2048)), block(kPairThreads);
    const uint32_t* r = (const uint32_t*)rec;
    auto* c = reinterpret_cast<const unsigned long long*>(ctr);
#define MTSV_PAIR_WAVE(W, M) hipLaunchKernelGGL((k_pair_wave<W, M>), grid, block, 0, s, r, n, n_reads, off, max_insert, list, c, val, add)
    if (mode == kPairProper) MTSV_PAIR_WAVE(6, kPairProper);
    else if (grain == kCollapseGrainTaxid) MTSV_PAIR_WAVE(4, kPairBoth);  // (BOTH and EITHER walk the same window)
    else MTSV_PAIR_WAVE(6, kPairBoth);
#undef MTSV_PAIR_WAVE
}

void launch_pair_heads(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, uint32_t* tile_cnt) {
    pair_check(grain, kPairBoth, tile);
    const uint32_t tiles = pair_tiles(n, tile);
    if (!tiles) return;
    if (grain == kCollapseGrainTaxid) hipLaunchKernelGGL(k_pair_heads<4>, dim3(tiles), dim3(kPairThreads), 0, s, (const uint32_t*)rec, n, tile, tile_cnt);
    else hipLaunchKernelGGL(k_pair_heads<6>, dim3(tiles), dim3(kPairThreads), 0, s, (const uint32_t*)rec, n, tile, tile_cnt);
}

void launch_pair_min(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, const uint32_t* tile_off, const uint32_t* val,
                     const uint32_t* add, uint32_t n_slots_cap, uint32_t* m, void* slot_rec) {
    pair_check(grain, kPairBoth, tile);
    const uint32_t tiles = pair_tiles(n, tile);
    if (!tiles) return;
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL(k_pair_min<4>, dim3(tiles), dim3(kPairThreads), 0, s, (const uint32_t*)rec, n, tile, tile_off, val, add, n_slots_cap, m, (uint4*)slot_rec);
    else
        hipLaunchKernelGGL(k_pair_min<6>, dim3(tiles), dim3(kPairThreads), 0, s, (const uint32_t*)rec, n, tile, tile_off, val, add, n_slots_cap, m, (uint4*)slot_rec);
}

void launch_pair_flags(hipStream_t s, const uint64_t* n_slots, uint32_t n_slots_cap, const void* slot_rec, uint32_t* m, uint32_t* flag_a, uint32_t* flag_b) {
    if (!n_slots_cap) return;
    hipLaunchKernelGGL(k_pair_flags, dim3(cdiv(n_slots_cap, kPairThreads)), dim3(kPairThreads), 0, s, reinterpret_cast<const unsigned long long*>(n_slots),
                       n_slots_cap, (const uint4*)slot_rec, m, flag_a, flag_b);
}

void launch_pair_write(hipStream_t s, const uint64_t* n_slots, uint32_t n_slots_cap, const void* slot_rec, const uint32_t* m, const uint32_t* pos_a,
                       const uint32_t* pos_b, uint32_t n_a, uint32_t n_b, void* out_a, void* out_b) {
    if (!n_slots_cap) return;
    hipLaunchKernelGGL(k_pair_write, dim3(cdiv(n_slots_cap, kPairThreads)), dim3(kPairThreads), 0, s, reinterpret_cast<const unsigned long long*>(n_slots),
                       n_slots_cap, (const uint4*)slot_rec, m, pos_a, pos_b, n_a, n_b, (uint4*)out_a, (uint4*)out_b);
}

void launch_pair_stats(hipStream_t s, const uint32_t* off, uint64_t n_pairs, const void* out, uint32_t n_out, uint64_t* ctr) {
    const uint64_t lanes = std::max<uint64_t>(n_pairs, n_out);
    if (!lanes) return;
    hipLaunchKernelGGL(k_pair_stats, dim3(std::min<uint32_t>(cdiv(lanes, kPairThreads), 1024)), dim3(kPairThreads), 0, s, off, n_pairs, (const uint32_t*)out, n_out,
                       reinterpret_cast<unsigned long long*>(ctr));
}

}  // namespace mtsv
