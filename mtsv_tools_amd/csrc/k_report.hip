// k_report.hip -- per-TaxID read counts of a pass (collapse.rs:43-62,120-146: what mtsv-collapse --report computes
// from the results text), from the pass's gathered hits while they are still in HBM.
//
// Per read with hits: summary = {tax_id -> smallest edit over the read's hits}; with m the smallest edit of the
// summary and `best` the number of its entries at m, every entry adds one to one counter of its TaxID:
//   only_hit (the summary has one entry) | only_best (at m, best == 1) | tied_best (at m) | not_best.
//
// Accumulation.  A pass lands millions of adds on as many addresses as the index has taxa, and a real sample puts
// most of them on a few: one global atomic per hit would serialise on those addresses (9-11 ns each, DESIGN.md
// section 5).  So a workgroup strides over its share of the reads and counts in LDS (u32: a read adds at most one to
// any counter and a pass holds fewer than 2^31 reads), lanes of a wavefront that reach the add with the first active
// lane's key go in as one add of their number, and the workgroup's non-zero counters go to the global u64 counters
// once, at its end.  Two tiers:
//   dense   4 * n_taxa counters in LDS, addressed by slot * 4 + category.  Up to kReportDenseTaxa taxa: 64 KiB of the
//           CU's 160 KiB per workgroup, so two workgroups (of up to 16 wavefronts each) stay resident per CU;
//   hashed  an open-addressing table of kReportHashSlots (key, count) pairs in LDS (32 KiB; fewer in tests); a key that
//           finds no place within kReportProbes steps is added to its global counter directly.
// Integer sums only: the result does not depend on how the reads were cut into passes, lanes or workgroups.
#include <hip/hip_runtime.h>

#include <string>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kReportThreads = 256, kReportMaxThreads = 1024;  // per workgroup: a small pass, a pass that fills the grid
constexpr uint32_t kReportGrid = 512;
constexpr uint32_t kReportProbes = 8;
constexpr uint32_t kReportEmpty = 0xffffffffu;
// reads of more hits than this are classified by their whole wavefront (a lane walking hundreds of hits alone while 63
// wait: what k_resolve avoids the same way)
constexpr uint32_t kReportCoop = 16;

struct ReportLds {
    uint32_t* cnt;   // dense: 4 * n_taxa counters; hashed: the slots' counts
    uint32_t* keys;  // hashed: the slots' keys
    uint32_t mask;   // hashed: slots - 1
    uint32_t* n_direct;  // trace only (else null): adds of this workgroup that went to the global counters directly
};

// (tax_id, edit) of a hit
__device__ inline uint2 hit_te(const DevHit* __restrict__ hits, uint64_t i) { return make_uint2(hits[i].tax_id, hits[i].edit); }

template <bool DENSE>
__device__ inline void lds_add(const ReportLds& s, unsigned long long* __restrict__ counts, uint32_t key, uint32_t c) {
    if (DENSE) {
        atomicAdd(&s.cnt[key], c);
        return;
    }
    uint32_t h = (key * 0x9E3779B1u) >> 20 & s.mask;
    for (uint32_t p = 0; p < kReportProbes; p++) {
        const uint32_t old = atomicCAS(&s.keys[h], kReportEmpty, key);
        if (old == kReportEmpty || old == key) {
            atomicAdd(&s.cnt[h], c);
            return;
        }
        h = (h + 1) & s.mask;
    }
    atomicAdd(&counts[key], (unsigned long long)c);
    if (s.n_direct) atomicAdd(s.n_direct, 1u);
}

// One to counter `cat` of the taxon: the lanes that arrive here together with the first active lane's key add their
// number at once (the reads of a skewed sample all carry the same key), the others add for themselves.
template <bool DENSE>
__device__ inline void count_one(const ReportLds& s, unsigned long long* __restrict__ counts, const uint32_t* __restrict__ taxa,
                                 uint32_t n_taxa, uint32_t tax_id, uint32_t cat) {
    const uint32_t slot = find_u32(taxa, n_taxa, tax_id);  // (its dense slot: the place among the index's TaxIDs)
    if (slot >= n_taxa) return;  // (cannot happen: every hit's TaxID comes from the index's bins)
    const uint32_t key = slot * 4 + cat;
    const uint32_t first = __builtin_amdgcn_readfirstlane(key);
    if (key == first) {
        const unsigned long long same = __ballot(1);
        if (lane_id() == (uint32_t)__builtin_ctzll(same)) lds_add<DENSE>(s, counts, key, (uint32_t)__popcll(same));
    } else {
        lds_add<DENSE>(s, counts, key, 1);
    }
}

constexpr uint32_t kOnlyHit = 0, kOnlyBest = 1, kTiedBest = 2, kNotBest = 3;

template <bool DENSE>
__global__ __launch_bounds__(kReportMaxThreads) void k_report(uint32_t n_reads, const uint32_t* __restrict__ strand_nout,
                                                           const uint32_t* __restrict__ out_off, const DevHit* __restrict__ hits,
                                                           const uint32_t* __restrict__ taxa, uint32_t n_taxa, uint32_t hash_slots,
                                                           unsigned long long* __restrict__ counts,
                                                           unsigned long long* __restrict__ total_reads,
                                                           unsigned long long* __restrict__ n_global) {
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t s_reads, s_global;
    ReportLds s;
    s.cnt = lds;
    s.keys = lds + hash_slots;
    s.mask = hash_slots - 1;
    s.n_direct = n_global ? &s_global : nullptr;
    const uint32_t n_cnt = DENSE ? 4 * n_taxa : hash_slots;
    for (uint32_t k = threadIdx.x; k < n_cnt; k += blockDim.x) {
        s.cnt[k] = 0;
        if (!DENSE) s.keys[k] = kReportEmpty;
    }
    if (threadIdx.x == 0) s_reads = s_global = 0;
    __syncthreads();

    const uint32_t lane = lane_id();
    uint32_t my_reads = 0;
    // (the loop bound is the same for every lane of the workgroup: the wavefront steps below need all 64)
    for (uint32_t r_base = blockIdx.x * blockDim.x; r_base < n_reads; r_base += gridDim.x * blockDim.x) {
        const uint32_t r = r_base + threadIdx.x;
        uint32_t n = 0;
        uint64_t b = 0;
        if (r < n_reads) {
            n = strand_nout[2 * r] + strand_nout[2 * r + 1];
            b = out_off[2 * r];
        }
        my_reads += n != 0;
        const bool big = n > kReportCoop;
        if (n == 1) {
            count_one<DENSE>(s, counts, taxa, n_taxa, hit_te(hits, b).x, kOnlyHit);
        } else if (n && !big) {
            uint32_t m = 0xffffffffu;
            for (uint32_t i = 0; i < n; i++) m = min(m, hit_te(hits, b + i).y);
            // entries at m wait until it is known whether another follows: `hold` is the first of them
            uint32_t nd = 0, best = 0, hold = 0;
            for (uint32_t i = 0; i < n; i++) {
                const uint2 hi = hit_te(hits, b + i);
                bool first = true;
                uint32_t emin = hi.y;
                for (uint32_t j = 0; j < n; j++) {
                    const uint2 hj = hit_te(hits, b + j);
                    if (j != i && hj.x == hi.x) {
                        first = first && j > i;
                        emin = min(emin, hj.y);
                    }
                }
                if (!first) continue;
                nd++;
                if (emin != m) {
                    count_one<DENSE>(s, counts, taxa, n_taxa, hi.x, kNotBest);
                } else if (++best == 1) {
                    hold = hi.x;
                } else {
                    if (best == 2) count_one<DENSE>(s, counts, taxa, n_taxa, hold, kTiedBest);
                    count_one<DENSE>(s, counts, taxa, n_taxa, hi.x, kTiedBest);
                }
            }
            if (best == 1) count_one<DENSE>(s, counts, taxa, n_taxa, hold, nd == 1 ? kOnlyHit : kOnlyBest);
        }
        // reads of many hits, one after the other, 64 hits a step
        for (unsigned long long bm = __ballot(big); bm; bm &= bm - 1) {
            const int l = __builtin_ctzll(bm);
            const uint32_t n_l = __builtin_amdgcn_readlane(n, l);
            const uint64_t b_l = ((uint64_t)__builtin_amdgcn_readlane((uint32_t)(b >> 32), l) << 32) | __builtin_amdgcn_readlane((uint32_t)b, l);
            uint32_t m = 0xffffffffu;
            for (uint32_t i = lane; i < n_l; i += kWave) m = min(m, hit_te(hits, b_l + i).y);
            for (int d = 32; d > 0; d >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, d));
            // first sweep: distinct TaxIDs, how many of them at m, and the entries above m (those are not_best whatever
            // the rest of the read holds)
            uint32_t nd = 0, best = 0;
            for (uint32_t base = 0; base < n_l; base += kWave) {
                const uint32_t i = base + lane;
                bool first = i < n_l;
                uint2 hi = make_uint2(0, 0);
                if (first) hi = hit_te(hits, b_l + i);
                uint32_t emin = hi.y;
                for (uint32_t j = 0; j < n_l; j++) {  // (every lane reads the same hit: one fetch per step)
                    const uint2 hj = hit_te(hits, b_l + j);
                    if (j != i && hj.x == hi.x) {
                        first = first && j > i;
                        emin = min(emin, hj.y);
                    }
                }
                nd += (uint32_t)__popcll(__ballot(first));
                best += (uint32_t)__popcll(__ballot(first && emin == m));
                if (first && emin != m) count_one<DENSE>(s, counts, taxa, n_taxa, hi.x, kNotBest);
            }
            // second sweep: the entries at m, each by the first of its TaxID's hits with that edit
            const uint32_t cat = nd == 1 ? kOnlyHit : best == 1 ? kOnlyBest : kTiedBest;
            for (uint32_t base = 0; base < n_l; base += kWave) {
                const uint32_t i = base + lane;
                uint2 hi = make_uint2(0, 0xffffffffu);
                if (i < n_l) hi = hit_te(hits, b_l + i);
                bool rep = i < n_l && hi.y == m;
                if (!__ballot(rep)) continue;
                for (uint32_t j = 0; j < base + kWave - 1 && j < n_l; j++) {
                    const uint2 hj = hit_te(hits, b_l + j);
                    if (j < i && hj.x == hi.x && hj.y == m) rep = false;
                }
                if (rep) count_one<DENSE>(s, counts, taxa, n_taxa, hi.x, cat);
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) my_reads += __shfl_down(my_reads, d);
    if (lane == 0 && my_reads) atomicAdd(&s_reads, my_reads);
    __syncthreads();
    // the workgroup's counters to the global ones: non-zero entries only
    for (uint32_t k = threadIdx.x; k < n_cnt; k += blockDim.x) {
        const uint32_t c = s.cnt[k];
        if (c) atomicAdd(&counts[DENSE ? k : s.keys[k]], (unsigned long long)c);
        if (c && n_global) atomicAdd(&s_global, 1u);
    }
    if (threadIdx.x == 0 && s_reads) atomicAdd(total_reads, (unsigned long long)s_reads);
    if (n_global) {  // (MTSV_TRACE: how many adds the pass made on the global counters)
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(n_global, (unsigned long long)s_global + (s_reads != 0));
    }
}

}  // namespace

void launch_report(hipStream_t s, uint32_t n_reads, const uint32_t* strand_nout, const uint32_t* out_off, const DevHit* hits,
                   const uint32_t* taxa, uint32_t n_taxa, bool dense, uint32_t hash_slots, uint64_t* counts, uint64_t* total_reads,
                   uint64_t* n_global) {
    if (!n_reads) return;
    if (!dense && (hash_slots < 16 || hash_slots > kReportHashSlots || (hash_slots & (hash_slots - 1))))
        throw std::runtime_error("internal: taxa report hash table of " + std::to_string(hash_slots) + " slots");
    if (dense && n_taxa > kReportDenseTaxa) throw std::runtime_error("internal: dense taxa report beyond its LDS budget");
    // Two workgroups per CU at most (256 CUs): every workgroup flushes its own counters, so more of them means more global
    // atomics per pass, not more speed.  What the kernel needs is wavefronts in flight -- a read is a chain of dependent
    // loads (its counts, its hits, ten steps of the binary search): on 10 M reads 2048 wavefronts took 1.15 ms, 4096 0.77,
    // 8192 and more 0.53 whatever the grid, with 0.9 to 3.6 M atomics alike -- so a pass that fills the grid runs workgroups
    // of 16 wavefronts, a smaller one a read per thread in workgroups of four.
    const uint32_t block = cdiv(n_reads, kReportThreads) > kReportGrid ? kReportMaxThreads : kReportThreads;
    const uint32_t grid = std::min<uint32_t>(cdiv(n_reads, block), kReportGrid);
    auto* c = reinterpret_cast<unsigned long long*>(counts);
    auto* t = reinterpret_cast<unsigned long long*>(total_reads);
    auto* g = reinterpret_cast<unsigned long long*>(n_global);
    if (dense)
        hipLaunchKernelGGL(k_report<true>, dim3(grid), dim3(block), 4 * n_taxa * sizeof(uint32_t), s, n_reads, strand_nout,
                           out_off, hits, taxa, n_taxa, 0u, c, t, g);
    else
        hipLaunchKernelGGL(k_report<false>, dim3(grid), dim3(block), 2 * hash_slots * sizeof(uint32_t), s, n_reads,
                           strand_nout, out_off, hits, taxa, n_taxa, hash_slots, c, t, g);
}

}  // namespace mtsv
