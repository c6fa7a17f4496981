// k_collapse.hip -- the assignments of a pass: per read one (tax_id, smallest edit) per distinct TaxID, ascending by
// TaxID (binner.rs:355-378, write_assignments; collapse.rs:269-297 across result files), from the pass's gathered hits
// while they are still in HBM.
//
// The key of a hit is tax_id << 32 | edit: with a read's keys sorted ascending, the record to keep is the first of every
// run of equal high words.  So: one kernel pair SORTS every read's keys into a key scratch that mirrors the hit array
// (key i of the scratch belongs to the read hit i belongs to) and writes a flag per key, "first of its TaxID"; the
// existing scan turns the flags into places; a flat kernel, a lane per key, WRITES the flagged keys as records.  The scan's
// total is the pass's record count.  No read is sorted twice and the write does not know about reads at all (DESIGN.md
// section 7 says why this and not count / scan / write per read).
//
// The sort by tiers of a read's hit count n:
//   lane       n <= lane_max (<= 16): a read per lane.  One hit: key and flag go straight out.  More: every key's place is
//              the number of the read's keys that sort before it (ties by position), counted pairwise -- the pattern of
//              k_report's classification, at most 16 x 16 cached loads and no array in registers;
//   wavefront  n <= wave_max (<= 64): the wavefront takes such a read together, a key per lane, and counts the same
//              places from the other lanes' registers (readlane), n steps;
//   listed     everything larger is appended to a list (one atomic per wavefront that has any) and k_collapse_heavy
//              takes the list a workgroup per read from a ticket, as k_coalesce_heavy does: up to lds_max (<= 4096) keys
//              sorted by a bitonic network in 32 KiB of LDS, more than that by the same network in the key scratch
//              itself (global memory, any n).  The kernel is a small fixed grid that finds an empty list and leaves.
// The network is the one whose merges all run upwards (the first step of a merge pairs i with i ^ (k - 1)), so that a
// count that is no power of two needs no padding: a pair whose upper index is past the end is skipped, as if +inf sat
// there already.
//
// Grains.  Everything above is written once, over a grain policy: the key made from a DevHit, its order, "same group", and
// the record written.  GrainTaxid is the 64-bit key above and the 16-byte record.  The two wide grains keep the GI and the
// offset (below 2^32 on the device: dev_index.hip refuses larger indexes), so their key is 128 bits, tax || gi in the high
// word and in the low word
//   long      offset || edit: the first of every run of equal tax || gi || offset carries the triple's smallest edit
//             (binner.rs:320-352);
//   taxid-gi  edit || offset: the first of every run of equal tax || gi carries the pair's smallest (edit, offset)
//             (collapse.rs:603-625);
// the record is 24 bytes (mtsv_assignment_gi).  A 16-byte key halves what 32 KiB of LDS hold: the LDS tier of the wide grains
// ends at kCollapseLdsKeysWide.
#include <hip/hip_runtime.h>

#include <string>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kCollapseThreads = 256;
constexpr uint32_t kCollapseGrid = 2048;
constexpr uint32_t kCollapseHeavyGrid = 128;

__device__ inline uint32_t key_tax(uint64_t k) { return (uint32_t)(k >> 32); }

__device__ inline uint64_t readlane64(uint64_t v, int l) {
    return ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), l) << 32) | __builtin_amdgcn_readlane((uint32_t)v, l);
}

struct alignas(16) Key128 {
    uint64_t hi, lo;
};
__device__ inline bool key_before(uint64_t a, uint64_t b) { return a < b; }
__device__ inline bool key_equal(uint64_t a, uint64_t b) { return a == b; }
__device__ inline uint64_t key_readlane(uint64_t v, int l) { return readlane64(v, l); }
__device__ inline bool key_before(const Key128& a, const Key128& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ inline bool key_equal(const Key128& a, const Key128& b) { return a.hi == b.hi && a.lo == b.lo; }
__device__ inline bool operator==(const Key128& a, const Key128& b) { return key_equal(a, b); }
__device__ inline bool operator!=(const Key128& a, const Key128& b) { return !key_equal(a, b); }
// (readlane returns an int: a wide key has GI or offset bits in bit 31 of a low dword, which must not be sign-extended into
//  the high one; the 64-bit key's low dword is an edit distance and keeps the code it had)
__device__ inline uint64_t readlane64u(uint64_t v, int l) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((uint32_t)v, l);
}
__device__ inline Key128 key_readlane(const Key128& v, int l) { return Key128{readlane64u(v.hi, l), readlane64u(v.lo, l)}; }  // four dwords a step

struct GrainTaxid {
    using Key = uint64_t;
    static constexpr uint32_t kLdsKeys = kCollapseLdsKeys;
    static __device__ inline Key key(const DevHit* __restrict__ hits, uint64_t i) { return (uint64_t)hits[i].tax_id << 32 | hits[i].edit; }
    static __device__ inline uint32_t group(Key k) { return key_tax(k); }  // keys of one record agree in this
    static __device__ inline void write(void* __restrict__ out, uint32_t at, Key k, uint64_t read) {  // mtsv_assignment
        reinterpret_cast<uint4*>(out)[at] = make_uint4((uint32_t)read, (uint32_t)(read >> 32), key_tax(k), (uint32_t)k);
    }
};
struct GrainLong {
    using Key = Key128;
    static constexpr uint32_t kLdsKeys = kCollapseLdsKeysWide;
    static __device__ inline Key key(const DevHit* __restrict__ hits, uint64_t i) {
        return Key{(uint64_t)hits[i].tax_id << 32 | hits[i].gi, (uint64_t)(uint32_t)hits[i].offset << 32 | hits[i].edit};
    }
    static __device__ inline Key group(const Key& k) { return Key{k.hi, k.lo >> 32}; }
    static __device__ inline void write(void* __restrict__ out, uint32_t at, const Key& k, uint64_t read) {  // mtsv_assignment_gi
        uint2* o = reinterpret_cast<uint2*>(out) + 3ull * at;
        o[0] = make_uint2((uint32_t)read, (uint32_t)(read >> 32));
        o[1] = make_uint2((uint32_t)(k.hi >> 32), (uint32_t)k.hi);
        o[2] = make_uint2((uint32_t)(k.lo >> 32), (uint32_t)k.lo);  // offset, edit
    }
};
struct GrainTaxidGi {
    using Key = Key128;
    static constexpr uint32_t kLdsKeys = kCollapseLdsKeysWide;
    static __device__ inline Key key(const DevHit* __restrict__ hits, uint64_t i) {
        return Key{(uint64_t)hits[i].tax_id << 32 | hits[i].gi, (uint64_t)hits[i].edit << 32 | (uint32_t)hits[i].offset};
    }
    static __device__ inline uint64_t group(const Key& k) { return k.hi; }
    static __device__ inline void write(void* __restrict__ out, uint32_t at, const Key& k, uint64_t read) {  // mtsv_assignment_gi
        uint2* o = reinterpret_cast<uint2*>(out) + 3ull * at;
        o[0] = make_uint2((uint32_t)read, (uint32_t)(read >> 32));
        o[1] = make_uint2((uint32_t)(k.hi >> 32), (uint32_t)k.hi);
        o[2] = make_uint2((uint32_t)k.lo, (uint32_t)(k.lo >> 32));  // offset, edit
    }
};

// the workgroup's tier counts to the global counters: one add per counter and workgroup
__device__ inline void add_tier_counts(uint32_t* s_cnt, const uint32_t (&mine)[3], unsigned long long* __restrict__ ctr) {
    for (int t = 0; t < 3; t++) {
        uint32_t c = mine[t];
        for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
        if (lane_id() == 0 && c) atomicAdd(&s_cnt[t], c);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&ctr[kCollapseCtrLane + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

template <class G>
__global__ __launch_bounds__(kCollapseThreads) void k_collapse_small(uint32_t n_reads, const uint32_t* __restrict__ strand_nout,
                                                                    const uint32_t* __restrict__ out_off, const DevHit* __restrict__ hits,
                                                                    uint32_t lane_max, uint32_t wave_max, typename G::Key* __restrict__ keys,
                                                                    uint32_t* __restrict__ flags, uint32_t* __restrict__ list,
                                                                    unsigned long long* __restrict__ ctr) {
    using Key = typename G::Key;
    __shared__ uint32_t s_cnt[3];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = lane_id();
    uint32_t mine[3] = {0, 0, 0};  // reads this lane saw go to the lane tier, the wavefront tier, the list
    // (the loop bound is the same for every lane of the workgroup: the wavefront steps below need all 64)
    for (uint32_t r_base = blockIdx.x * blockDim.x; r_base < n_reads; r_base += gridDim.x * blockDim.x) {
        const uint32_t r = r_base + threadIdx.x;
        uint32_t n = 0;
        uint64_t b = 0;
        if (r < n_reads) {
            n = strand_nout[2 * r] + strand_nout[2 * r + 1];
            b = out_off[2 * r];
        }
        const bool by_wave = n > lane_max && n <= wave_max;
        const bool listed = n > lane_max && n > wave_max;
        mine[0] += n != 0 && n <= lane_max;
        mine[1] += by_wave;
        mine[2] += listed;
        if (n == 1) {
            keys[b] = G::key(hits, b);
            flags[b] = 1;
        } else if (n && n <= lane_max) {
            for (uint32_t i = 0; i < n; i++) {
                const Key ki = G::key(hits, b + i);
                uint32_t place = 0;
                bool head = true;
                for (uint32_t j = 0; j < n; j++) {
                    const Key kj = G::key(hits, b + j);
                    const bool before = key_before(kj, ki) || (key_equal(kj, ki) && j < i);
                    place += before;
                    head = head && !(before && G::group(kj) == G::group(ki));
                }
                keys[b + place] = ki;
                flags[b + place] = head;
            }
        }
        // reads for the whole wavefront, one after the other: a key per lane, its place counted from the other lanes' keys
        for (unsigned long long bm = __ballot(by_wave); bm; bm &= bm - 1) {
            const int l = __builtin_ctzll(bm);
            const uint32_t n_l = __builtin_amdgcn_readlane(n, l);
            const uint64_t b_l = readlane64(b, l);
            const Key ki = lane < n_l ? G::key(hits, b_l + lane) : Key{};
            uint32_t place = 0;
            bool head = true;
            for (uint32_t j = 0; j < n_l; j++) {
                const Key kj = key_readlane(ki, (int)j);
                const bool before = key_before(kj, ki) || (key_equal(kj, ki) && j < lane);
                place += before;
                head = head && !(before && G::group(kj) == G::group(ki));
            }
            if (lane < n_l) {
                keys[b_l + place] = ki;
                flags[b_l + place] = head;
            }
        }
        // the rest goes on the list: one add on its counter per wavefront that has any
        const unsigned long long lm = __ballot(listed);
        if (lm) {
            const int first = __builtin_ctzll(lm);
            uint32_t at = 0;
            if ((int)lane == first) at = (uint32_t)atomicAdd(&ctr[kCollapseCtrList], (unsigned long long)__popcll(lm));
            at = __builtin_amdgcn_readlane(at, first);
            if (listed) list[at + (uint32_t)__popcll(lm & ((1ull << lane) - 1))] = r;
        }
    }
    add_tier_counts(s_cnt, mine, ctr);
}

// a[0 .. n) ascending, by the whole workgroup; a in LDS or in global memory.  Every step is followed by a barrier.
template <class T>
__device__ inline void block_bitonic(T* a, uint32_t n) {
    uint64_t N = 1;
    while (N < n) N <<= 1;
    for (uint64_t k = 2; k <= N; k <<= 1) {
        for (uint64_t j = k >> 1; j > 0; j >>= 1) {
            const bool flip = j == (k >> 1);  // the first step of a merge: i against its mirror image in the block of k
            for (uint64_t t = threadIdx.x; t < (N >> 1); t += blockDim.x) {
                const uint64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // bit j of i is clear
                const uint64_t p = flip ? (i ^ (k - 1)) : (i | j);
                if (p < n) {
                    const T x = a[i], y = a[p];
                    if (key_before(y, x)) {
                        a[i] = y;
                        a[p] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

template <class G>
__global__ __launch_bounds__(kCollapseThreads) void k_collapse_heavy(const uint32_t* __restrict__ strand_nout, const uint32_t* __restrict__ out_off,
                                                                    const DevHit* __restrict__ hits, uint32_t lds_max, typename G::Key* keys,
                                                                    uint32_t* __restrict__ flags, const uint32_t* __restrict__ list,
                                                                    unsigned long long* ctr) {
    using Key = typename G::Key;
    __shared__ Key s_keys[G::kLdsKeys];  // 32 KiB in every grain
    __shared__ uint32_t s_item;
    const uint32_t n_list = (uint32_t)ctr[kCollapseCtrList];
    uint32_t in_lds = 0, in_global = 0;  // (thread 0 counts)
    for (;;) {
        if (threadIdx.x == 0) s_item = (uint32_t)atomicAdd(&ctr[kCollapseCtrTicket], 1ull);
        __syncthreads();
        const uint32_t item = s_item;
        __syncthreads();  // (everyone has read the ticket before the next one overwrites it)
        if (item >= n_list) break;
        const uint32_t r = list[item];
        const uint32_t n = strand_nout[2 * r] + strand_nout[2 * r + 1];
        const uint64_t b = out_off[2 * r];
        if (n <= lds_max) {
            in_lds++;
            for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) s_keys[i] = G::key(hits, b + i);
            __syncthreads();
            block_bitonic(s_keys, n);
            for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
                const Key k = s_keys[i];
                keys[b + i] = k;
                flags[b + i] = i == 0 || G::group(s_keys[i - 1]) != G::group(k);
            }
            __syncthreads();  // (the next read's keys overwrite these)
        } else {
            in_global++;
            Key* g = keys + b;
            for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) g[i] = G::key(hits, b + i);
            __syncthreads();
            block_bitonic(g, n);
            for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) flags[b + i] = i == 0 || G::group(g[i - 1]) != G::group(g[i]);
        }
    }
    if (threadIdx.x == 0 && in_lds) atomicAdd(&ctr[kCollapseCtrLds], (unsigned long long)in_lds);
    if (threadIdx.x == 0 && in_global) atomicAdd(&ctr[kCollapseCtrGlobal], (unsigned long long)in_global);
}

// a lane per key: the flagged ones become records at the places the scan gave them
template <class G>
__global__ __launch_bounds__(kCollapseThreads) void k_collapse_write(uint32_t n_hits, const DevHit* __restrict__ hits,
                                                                    const typename G::Key* __restrict__ keys, const uint32_t* __restrict__ flags,
                                                                    const uint32_t* __restrict__ place, void* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kCollapseThreads + threadIdx.x;
    if (i >= n_hits || !flags[i]) return;
    const typename G::Key k = keys[i];
    const uint64_t read = hits[i].read;
    G::write(out, place[i], k, read);
}

template <class G>
void launch_collapse_grain(hipStream_t s, uint32_t n_reads, const uint32_t* strand_nout, const uint32_t* out_off, const DevHit* hits, uint32_t n_hits,
                           uint32_t lane_max, uint32_t wave_max, uint32_t lds_max, void* keys_v, uint32_t* flags, uint32_t* place, uint64_t* tile_sums,
                           uint32_t* list, uint64_t* ctr, void* out) {
    if (lane_max < 1 || lane_max > kCollapseLaneMax || wave_max > kWave || lds_max < 2 || lds_max > G::kLdsKeys || (lds_max & (lds_max - 1)))
        throw std::runtime_error("internal: collapse thresholds " + std::to_string(lane_max) + " / " + std::to_string(wave_max) + " / " +
                                 std::to_string(lds_max));
    launch_clear_counters(s, ctr, (1ull << kCollapseCounters) - 1);
    if (!n_reads || !n_hits) return;  // (the total stays 0)
    auto* c = reinterpret_cast<unsigned long long*>(ctr);
    auto* keys = reinterpret_cast<typename G::Key*>(keys_v);
    hipLaunchKernelGGL(k_collapse_small<G>, dim3(std::min(cdiv(n_reads, kCollapseThreads), kCollapseGrid)), dim3(kCollapseThreads), 0, s, n_reads,
                       strand_nout, out_off, hits, lane_max, wave_max, keys, flags, list, c);
    hipLaunchKernelGGL(k_collapse_heavy<G>, dim3(kCollapseHeavyGrid), dim3(kCollapseThreads), 0, s, strand_nout, out_off, hits, lds_max, keys, flags,
                       list, c);
    launch_scan(s, flags, n_hits, tile_sums, ctr + kCollapseCtrTotal, place);
    hipLaunchKernelGGL(k_collapse_write<G>, dim3(cdiv(n_hits, kCollapseThreads)), dim3(kCollapseThreads), 0, s, n_hits, hits, keys, flags, place, out);
}

}  // namespace

void launch_collapse(hipStream_t s, int grain, uint32_t n_reads, const uint32_t* strand_nout, const uint32_t* out_off, const DevHit* hits,
                     uint32_t n_hits, uint32_t lane_max, uint32_t wave_max, uint32_t lds_max, void* keys, uint32_t* flags, uint32_t* place,
                     uint64_t* tile_sums, uint32_t* list, uint64_t* ctr, void* out) {
    switch (grain) {
        case kCollapseGrainTaxid:
            return launch_collapse_grain<GrainTaxid>(s, n_reads, strand_nout, out_off, hits, n_hits, lane_max, wave_max, lds_max, keys, flags, place,
                                                     tile_sums, list, ctr, out);
        case kCollapseGrainTaxidGi:
            return launch_collapse_grain<GrainTaxidGi>(s, n_reads, strand_nout, out_off, hits, n_hits, lane_max, wave_max, lds_max, keys, flags, place,
                                                       tile_sums, list, ctr, out);
        case kCollapseGrainLong:
            return launch_collapse_grain<GrainLong>(s, n_reads, strand_nout, out_off, hits, n_hits, lane_max, wave_max, lds_max, keys, flags, place,
                                                    tile_sums, list, ctr, out);
    }
    throw std::runtime_error("internal: collapse grain " + std::to_string(grain));
}

}  // namespace mtsv
