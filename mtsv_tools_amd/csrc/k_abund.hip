// k_abund.hip -- abundance by expectation-maximisation over a sorted list of assignment records (abund.hip, mtsv_fold_abundance;
// the definition is in include/mtsv_amd.h).
//
// PREPARE, once per call, record-parallel in the tile scaffold of k_tile.hpp (the scheme in full is there).  Two kinds of
// segments are counted at once, READS and RUNS (a run: the records of one (read, tax_id) -- the wide grains repeat a TaxID); the
// run heads are the scaffold's second kind, with cells of their own:
//   k_abund_heads  the read heads and the run heads of every tile                      (then launch_scan, twice)
//   k_abund_min    two segmented minima of edit, m[read slot] and e_run[run slot].  Heads write what is known of their read
//                  and run.
//   k_abund_flag   a lane per run: it ENTERS when e - m <= slack                          (then launch_scan: the entries' places)
//   k_abund_write  a lane per run: the entry -- the place of its TaxID in the union (find_u32 once here, not per iteration), the
//                  difference to the read's best clipped to the weight table as a byte, e -- and the per-taxon counts; the lane
//                  of a read's first run writes the read's offset and lists the read when it has more than lane_max entries.
// An ITERATION then streams about 5 bytes per entry (slot and d) instead of the 16 or 24 of a record; the masses, 8 bytes per
// TaxID of the union, stay in L2:
//   k_abund_step   persistent, grid-striding.  A lane takes each short read and walks its entries twice (the sum of the x, then
//                  the shares); a wavefront takes each listed read, strides it, reduces the sum by shuffles and strides again.
//                  A sample puts most mass on a few taxa, and global atomics on one address serialise (the
//                  head of k_report.hip), so with DENSE the adds go to 64-bit counters of the workgroup in LDS (up to 8192: 64 KiB
//                  of the CU's 160, two workgroups resident) and every non-zero counter is flushed with one global add at the
//                  workgroup's end.  Without it every add is a global 64-bit atomic add.  All adds are integer: same bits.
//   k_abund_delta  L1 of the change, the new masses become the current ones, the next are zeroed.
//   k_abund_final  the hard assignment in the same two tiers: arg-max on (x, first entry), i.e. the smallest TaxID.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "k_tile.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kAbundThreads = 256;
constexpr uint32_t kAbundWaves = kAbundThreads / kWave;
constexpr uint32_t kAbundStretchMax = kAbundTileMax / kAbundThreads;
static_assert(kAbundStretchMax <= 32, "the heads of a lane's stretch are kept as bits of one word");
static_assert(kAbundTileMax < (1u << 16), "two head counts of a tile share a word");
static_assert(kAbundDenseMax * sizeof(unsigned long long) <= 65536, "the dense counters fit the LDS of one workgroup");

// a read head: the read differs from the predecessor's; a run head, the second kind: the read or the tax_id does
struct AbundKey {
    uint64_t read;
    uint32_t tax;
};
template <uint32_t W>
struct AbundHead {
    const uint32_t* __restrict__ rec;
    __device__ AbundKey key(uint64_t i) const { return AbundKey{rec_read_of<W>(rec, i), rec[i * W + 2]}; }
    __device__ static uint32_t head(const AbundKey& prev, const AbundKey& cur) {
        const bool r = prev.read != cur.read;
        return (uint32_t)r | (uint32_t)(r || prev.tax != cur.tax) << 1;
    }
};

template <uint32_t W>
__global__ __launch_bounds__(kAbundThreads) void k_abund_heads(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, uint32_t* __restrict__ cnt_r,
                                                              uint32_t* __restrict__ cnt_p) {
    __shared__ uint32_t wsum[kAbundWaves];
    const auto t = tile_lane<kAbundThreads, 2>(n, tile, wsum, AbundHead<W>{rec});
    if (threadIdx.x == 0) {
        cnt_r[blockIdx.x] = t.total;
        cnt_p[blockIdx.x] = t.total2;
    }
}

template <uint32_t W>
__global__ __launch_bounds__(kAbundThreads) void k_abund_min(const uint32_t* __restrict__ rec, uint32_t n, uint32_t tile, const uint32_t* __restrict__ off_r,
                                                            const uint32_t* __restrict__ off_p, uint32_t n_reads, uint32_t n_runs, uint32_t* __restrict__ m,
                                                            uint32_t* __restrict__ e_run, unsigned long long* __restrict__ read_id,
                                                            uint32_t* __restrict__ read_first, uint32_t* __restrict__ run_tax,
                                                            uint32_t* __restrict__ run_read) {
    __shared__ uint32_t wsum[kAbundWaves];
    __shared__ uint32_t smin_r[kAbundTileMax + 1], smin_p[kAbundTileMax + 1];  // by rank among the tile's heads of the kind
    for (uint32_t r = threadIdx.x; r <= tile; r += kAbundThreads) {
        smin_r[r] = 0xffffffffu;
        smin_p[r] = 0xffffffffu;
    }
    const auto t = tile_lane<kAbundThreads, 2>(n, tile, wsum, AbundHead<W>{rec});
    // the heads before the tile: rank r is slot base + r - 1 (a list begins with a head of both kinds: base + r >= 1)
    const uint32_t base_r = off_r[blockIdx.x], base_p = off_p[blockIdx.x];
    for (uint32_t k = 0; k < t.ipt; k++) {  // (ipt is the same in every lane)
        const bool act = t.p0 + k < t.p1;
        uint32_t rr = 0, rp = 0, e = 0;
        if (act) {
            const uint64_t i = t.i0 + t.p0 + k;
            rr = tile_rank(t.heads, t.before, k);
            rp = tile_rank(t.heads2, t.before2, k);
            e = rec[i * W + W - 1];
            const uint64_t slot_r = (uint64_t)base_r + rr - 1, slot_p = (uint64_t)base_p + rp - 1;
            if ((t.heads2 >> k & 1) && slot_p < n_runs && slot_r < n_reads) {
                run_tax[slot_p] = rec[i * W + 2];
                run_read[slot_p] = (uint32_t)slot_r;
                if (t.heads >> k & 1) {
                    read_id[slot_r] = rec_read_of<W>(rec, i);
                    read_first[slot_r] = (uint32_t)slot_p;
                }
            }
        }
        seg_lds_reduce<false>(smin_r, act, rr, e);
        seg_lds_reduce<false>(smin_p, act, rp, e);
    }
    __syncthreads();
    tile_flush<kAbundThreads, 0>(t, n, base_r, n_reads, AbundHead<W>{rec}, [&](uint64_t slot, uint32_t r, bool shared) {
        const uint32_t v = smin_r[r];
        if (shared) atomicMin(&m[slot], v);
        else m[slot] = v;
    });
    tile_flush<kAbundThreads, 1>(t, n, base_p, n_runs, AbundHead<W>{rec}, [&](uint64_t slot, uint32_t r, bool shared) {
        const uint32_t v = smin_p[r];
        if (shared) atomicMin(&e_run[slot], v);
        else e_run[slot] = v;
    });
}

__global__ __launch_bounds__(kAbundThreads) void k_abund_flag(uint32_t n_runs, const uint32_t* __restrict__ e_run, const uint32_t* __restrict__ m,
                                                             const uint32_t* __restrict__ run_read, uint32_t slack, uint32_t* __restrict__ flag) {
    const uint64_t p = (uint64_t)blockIdx.x * kAbundThreads + threadIdx.x;
    if (p >= n_runs) return;
    const uint32_t e = e_run[p], best = m[run_read[p]];
    flag[p] = e >= best && e - best <= slack ? 1u : 0u;  // (e >= best always: m is the minimum over the read's runs)
}

__global__ __launch_bounds__(kAbundThreads) void k_abund_write(uint32_t n_reads, uint32_t n_runs, const uint32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ e_run, const uint32_t* __restrict__ m,
                                                              const uint32_t* __restrict__ run_tax, const uint32_t* __restrict__ run_read,
                                                              const uint32_t* __restrict__ read_first, const uint32_t* __restrict__ u_tax, uint32_t n_union,
                                                              uint32_t n_w, uint32_t lane_max, uint32_t* __restrict__ read_off,
                                                              uint32_t* __restrict__ ent_slot, uint8_t* __restrict__ ent_d, uint32_t* __restrict__ ent_e,
                                                              uint32_t* __restrict__ any, uint32_t* __restrict__ uniq, uint32_t* __restrict__ list,
                                                              unsigned long long* __restrict__ ctr) {
    const uint64_t p = (uint64_t)blockIdx.x * kAbundThreads + threadIdx.x;
    if (p >= n_runs) return;
    const uint32_t r = run_read[p];
    if (r >= n_reads) return;  // (never: k_abund_min numbers the reads below n_reads)
    const uint32_t first = read_first[r];
    const uint32_t next_first = r + 1 < n_reads ? read_first[r + 1] : n_runs;
    if (first > p || next_first > n_runs || next_first <= p) return;  // (never: the runs of a read are consecutive)
    const uint32_t lo = off[first], hi = off[next_first], cnt = hi - lo;
    const uint32_t n_entries = off[n_runs];
    if (p == first) {
        read_off[r] = lo;
        if (r + 1 == n_reads) read_off[n_reads] = hi;
        if (cnt >= kAbundEntriesMax) atomicAdd(&ctr[kAbundCtrLong], 1ull);
        else if (cnt > lane_max) {
            const unsigned long long at = atomicAdd(&ctr[kAbundCtrList], 1ull);
            if (at < n_reads) list[at] = r;
        }
    }
    const uint32_t j = off[p];
    if (off[p + 1] == j || j >= n_entries) return;  // (the run does not enter)
    const uint32_t e = e_run[p], d = e - m[r];
    const uint32_t slot = find_u32(u_tax, n_union, run_tax[p]);
    ent_d[j] = (uint8_t)min(d, n_w);
    ent_e[j] = e;
    if (slot >= n_union) {
        ent_slot[j] = 0;  // (the call fails on the counter before an iteration reads this)
        atomicAdd(&ctr[kAbundCtrMissing], 1ull);
        return;
    }
    ent_slot[j] = slot;
    atomicAdd(&any[slot], 1u);
    if (cnt == 1) atomicAdd(&uniq[slot], 1u);
}

__global__ __launch_bounds__(kAbundThreads) void k_abund_init(uint32_t n_union, const uint32_t* __restrict__ any, unsigned long long start,
                                                             unsigned long long* __restrict__ mass, unsigned long long* __restrict__ next) {
    const uint64_t i = (uint64_t)blockIdx.x * kAbundThreads + threadIdx.x;
    if (i >= n_union) return;
    mass[i] = any[i] ? start : 0ull;
    next[i] = 0;
}

// steps 1, 3 and 4 of the definition
__device__ inline unsigned long long abund_x(unsigned long long a, uint32_t d, const uint32_t* __restrict__ w) {
    return d == 0 ? a >> 16 : __umul64hi(a, (unsigned long long)w[d - 1] << 32) >> 16;
}
__device__ inline unsigned long long abund_x_prior(uint32_t d, const uint32_t* __restrict__ w) { return d == 0 ? 1ull << 15 : (unsigned long long)(w[d - 1] >> 17); }
__device__ inline unsigned long long abund_share(unsigned long long x, unsigned long long s) {
    return (unsigned long long)(((double)x / (double)s) * 4294967296.0);
}

__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// x of entry j under the masses, or under the uniform prior
__device__ inline unsigned long long abund_x_of(const AbundEntries& en, const unsigned long long* __restrict__ mass, uint32_t j, bool prior) {
    const uint32_t d = en.ent_d[j];
    return prior ? abund_x_prior(d, en.w) : abund_x(mass[en.ent_slot[j]], d, en.w);
}

template <bool DENSE>
__global__ __launch_bounds__(kAbundThreads) void k_abund_step(AbundEntries en, const unsigned long long* __restrict__ mass, unsigned long long* __restrict__ next) {
    extern __shared__ unsigned long long acc[];  // DENSE: n_union counters
    if (DENSE) {
        for (uint32_t i = threadIdx.x; i < en.n_union; i += kAbundThreads) acc[i] = 0;
        __syncthreads();
    }
    auto add = [&](uint32_t slot, unsigned long long q) {
        if (!q || slot >= en.n_union) return;
        if (DENSE) atomicAdd(&acc[slot], q);
        else atomicAdd(&next[slot], q);
    };
    const uint64_t n_threads = (uint64_t)gridDim.x * kAbundThreads, me = (uint64_t)blockIdx.x * kAbundThreads + threadIdx.x;
    // ---- a lane per short read ----
    for (uint64_t r = me; r < en.n_reads; r += n_threads) {
        const uint32_t lo = en.read_off[r], hi = en.read_off[r + 1];
        if (hi - lo > en.lane_max) continue;
        unsigned long long s = 0;
        for (uint32_t j = lo; j < hi; j++) s += abund_x_of(en, mass, j, false);
        const bool prior = s == 0;
        if (prior)
            for (uint32_t j = lo; j < hi; j++) s += abund_x_of(en, mass, j, true);
        if (!s) continue;  // (never: a read's best entry has d = 0)
        for (uint32_t j = lo; j < hi; j++) add(en.ent_slot[j], abund_share(abund_x_of(en, mass, j, prior), s));
    }
    // ---- a wavefront per listed read ----
    const uint64_t n_waves = n_threads / kWave;
    for (uint64_t k = me / kWave; k < en.n_list; k += n_waves) {  // (k is the same in every lane of the wavefront)
        const uint32_t r = en.list[k];
        if (r >= en.n_reads) continue;
        const uint32_t lo = en.read_off[r], hi = en.read_off[r + 1];
        unsigned long long s = 0;
        for (uint32_t j = lo + lane_id(); j < hi; j += kWave) s += abund_x_of(en, mass, j, false);
        s = wave_sum_u64(s);
        const bool prior = s == 0;
        if (prior) {
            for (uint32_t j = lo + lane_id(); j < hi; j += kWave) s += abund_x_of(en, mass, j, true);
            s = wave_sum_u64(s);
        }
        if (!s) continue;
        for (uint32_t j = lo + lane_id(); j < hi; j += kWave) add(en.ent_slot[j], abund_share(abund_x_of(en, mass, j, prior), s));
    }
    if (DENSE) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < en.n_union; i += kAbundThreads) {
            const unsigned long long v = acc[i];
            if (v) atomicAdd(&next[i], v);
        }
    }
}

__global__ __launch_bounds__(kAbundThreads) void k_abund_delta(uint32_t n_union, unsigned long long* __restrict__ mass, unsigned long long* __restrict__ next,
                                                              unsigned long long* __restrict__ l1) {
    const uint64_t n_threads = (uint64_t)gridDim.x * kAbundThreads;
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kAbundThreads + threadIdx.x; i < n_union; i += n_threads) {
        const unsigned long long a = mass[i], b = next[i];
        sum += a > b ? a - b : b - a;
        mass[i] = b;
        next[i] = 0;
    }
    sum = wave_sum_u64(sum);
    if (lane_id() == 0 && sum) atomicAdd(l1, sum);
}

__global__ __launch_bounds__(kAbundThreads) void k_abund_final(AbundEntries en, const unsigned long long* __restrict__ mass, const uint32_t* __restrict__ ent_e,
                                                              const unsigned long long* __restrict__ read_id, const uint32_t* __restrict__ u_tax,
                                                              uint32_t* __restrict__ out, uint32_t* __restrict__ assigned) {
    const uint64_t n_threads = (uint64_t)gridDim.x * kAbundThreads, me = (uint64_t)blockIdx.x * kAbundThreads + threadIdx.x;
    auto put = [&](uint32_t r, uint32_t j) {
        const unsigned long long read = read_id[r];
        *reinterpret_cast<uint4*>(out + (uint64_t)r * 4) = make_uint4((uint32_t)read, (uint32_t)(read >> 32), u_tax[en.ent_slot[j]], ent_e[j]);
    };
    // ---- a lane per short read; the loop's bound is the wavefront's, for the ballots ----
    for (uint64_t r = me; r - lane_id() < en.n_reads; r += n_threads) {
        bool ok = false;
        uint32_t slot = 0;
        if (r < en.n_reads) {
            const uint32_t lo = en.read_off[r], hi = en.read_off[r + 1];
            if (hi > lo && hi - lo <= en.lane_max) {
                unsigned long long s = 0;
                for (uint32_t j = lo; j < hi; j++) s += abund_x_of(en, mass, j, false);
                const bool prior = s == 0;
                unsigned long long best = 0;
                uint32_t at = lo;
                for (uint32_t j = lo; j < hi; j++) {
                    const unsigned long long x = abund_x_of(en, mass, j, prior);
                    if (x > best) {  // (entries ascend by TaxID: the first of equals is the smallest)
                        best = x;
                        at = j;
                    }
                }
                slot = en.ent_slot[at];
                ok = slot < en.n_union;
                if (ok) put((uint32_t)r, at);
            }
        }
        // the reads of the wavefront to their taxa, taxon by taxon: the lanes that hold the taxon of the first lane still waiting
        // add their number at once
        unsigned long long todo = __ballot(ok);
        while (todo) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
            const uint32_t s0 = (uint32_t)__shfl((int)slot, (int)leader);
            const unsigned long long same = __ballot(ok && slot == s0);
            if (lane_id() == leader) atomicAdd(&assigned[s0], (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
    // ---- a wavefront per listed read ----
    const uint64_t n_waves = n_threads / kWave;
    for (uint64_t k = me / kWave; k < en.n_list; k += n_waves) {
        const uint32_t r = en.list[k];
        if (r >= en.n_reads) continue;
        const uint32_t lo = en.read_off[r], hi = en.read_off[r + 1];
        if (hi <= lo) continue;
        unsigned long long s = 0;
        for (uint32_t j = lo + lane_id(); j < hi; j += kWave) s += abund_x_of(en, mass, j, false);
        const bool prior = wave_sum_u64(s) == 0;
        unsigned long long best = 0;
        uint32_t at = 0xffffffffu;  // (a lane without an entry, or whose x are all zero, loses to every entry)
        for (uint32_t j = lo + lane_id(); j < hi; j += kWave) {
            const unsigned long long x = abund_x_of(en, mass, j, prior);
            if (at == 0xffffffffu || x > best) {
                best = x;
                at = j;
            }
        }
        for (int d = kWave / 2; d > 0; d >>= 1) {
            const unsigned long long ox = __shfl_xor(best, d);
            const uint32_t oat = (uint32_t)__shfl_xor((int)at, d);
            if (oat != 0xffffffffu && (at == 0xffffffffu || ox > best || (ox == best && oat < at))) {
                best = ox;
                at = oat;
            }
        }
        if (lane_id() == 0 && at >= lo && at < hi) {
            const uint32_t slot = en.ent_slot[at];
            if (slot < en.n_union) {
                put(r, at);
                atomicAdd(&assigned[slot], 1u);
            }
        }
    }
}

void abund_check(int grain, uint32_t tile) {
    if (grain != kCollapseGrainTaxid && grain != kCollapseGrainTaxidGi && grain != kCollapseGrainLong)
        throw std::runtime_error("internal: abundance at grain " + std::to_string(grain));
    if (tile < 64 || tile > kAbundTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: abundance tile of " + std::to_string(tile) + " records");
}

}  // namespace

uint32_t abund_tiles(uint64_t n, uint32_t tile) { return cdiv(n, tile); }

void launch_abund_heads(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, uint32_t* cnt_r, uint32_t* cnt_p) {
    abund_check(grain, tile);
    const uint32_t tiles = abund_tiles(n, tile);
    if (!tiles) return;
    if (grain == kCollapseGrainTaxid) hipLaunchKernelGGL(k_abund_heads<4>, dim3(tiles), dim3(kAbundThreads), 0, s, (const uint32_t*)rec, n, tile, cnt_r, cnt_p);
    else hipLaunchKernelGGL(k_abund_heads<6>, dim3(tiles), dim3(kAbundThreads), 0, s, (const uint32_t*)rec, n, tile, cnt_r, cnt_p);
}

void launch_abund_min(hipStream_t s, int grain, const void* rec, uint32_t n, uint32_t tile, const uint32_t* off_r, const uint32_t* off_p,
                      uint32_t n_reads, uint32_t n_runs, uint32_t* m, uint32_t* e_run, uint64_t* read_id, uint32_t* read_first, uint32_t* run_tax,
                      uint32_t* run_read) {
    abund_check(grain, tile);
    const uint32_t tiles = abund_tiles(n, tile);
    if (!tiles || !n_reads || !n_runs) return;
    auto* ids = reinterpret_cast<unsigned long long*>(read_id);
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL(k_abund_min<4>, dim3(tiles), dim3(kAbundThreads), 0, s, (const uint32_t*)rec, n, tile, off_r, off_p, n_reads, n_runs, m, e_run, ids,
                           read_first, run_tax, run_read);
    else
        hipLaunchKernelGGL(k_abund_min<6>, dim3(tiles), dim3(kAbundThreads), 0, s, (const uint32_t*)rec, n, tile, off_r, off_p, n_reads, n_runs, m, e_run, ids,
                           read_first, run_tax, run_read);
}

void launch_abund_flag(hipStream_t s, uint32_t n_runs, const uint32_t* e_run, const uint32_t* m, const uint32_t* run_read, uint32_t slack,
                       uint32_t* flag) {
    if (!n_runs) return;
    hipLaunchKernelGGL(k_abund_flag, dim3(cdiv(n_runs, kAbundThreads)), dim3(kAbundThreads), 0, s, n_runs, e_run, m, run_read, slack, flag);
}

void launch_abund_write(hipStream_t s, uint32_t n_reads, uint32_t n_runs, const uint32_t* off, const uint32_t* e_run, const uint32_t* m,
                        const uint32_t* run_tax, const uint32_t* run_read, const uint32_t* read_first, const uint32_t* u_tax, uint32_t n_union,
                        uint32_t n_w, uint32_t lane_max, uint32_t* read_off, uint32_t* ent_slot, uint8_t* ent_d, uint32_t* ent_e, uint32_t* any,
                        uint32_t* uniq, uint32_t* list, uint64_t* ctr) {
    if (!n_runs || !n_reads) return;
    hipLaunchKernelGGL(k_abund_write, dim3(cdiv(n_runs, kAbundThreads)), dim3(kAbundThreads), 0, s, n_reads, n_runs, off, e_run, m, run_tax, run_read,
                       read_first, u_tax, n_union, n_w, lane_max, read_off, ent_slot, ent_d, ent_e, any, uniq, list, reinterpret_cast<unsigned long long*>(ctr));
}

void launch_abund_init(hipStream_t s, uint32_t n_union, const uint32_t* any, uint64_t start, uint64_t* mass, uint64_t* next) {
    if (!n_union) return;
    hipLaunchKernelGGL(k_abund_init, dim3(cdiv(n_union, kAbundThreads)), dim3(kAbundThreads), 0, s, n_union, any, (unsigned long long)start,
                       reinterpret_cast<unsigned long long*>(mass), reinterpret_cast<unsigned long long*>(next));
}

void launch_abund_step(hipStream_t s, uint32_t blocks, bool dense, const AbundEntries& en, const uint64_t* mass, uint64_t* next) {
    if (!en.n_reads || !blocks) return;
    if (dense && en.n_union > kAbundDenseMax) throw std::runtime_error("internal: dense abundance counters for " + std::to_string(en.n_union) + " TaxIDs");
    auto* a = reinterpret_cast<const unsigned long long*>(mass);
    auto* b = reinterpret_cast<unsigned long long*>(next);
    if (dense) hipLaunchKernelGGL(k_abund_step<true>, dim3(blocks), dim3(kAbundThreads), en.n_union * sizeof(unsigned long long), s, en, a, b);
    else hipLaunchKernelGGL(k_abund_step<false>, dim3(blocks), dim3(kAbundThreads), 0, s, en, a, b);
}

void launch_abund_delta(hipStream_t s, uint32_t n_union, uint64_t* mass, uint64_t* next, uint64_t* l1) {
    if (!n_union) return;
    const uint32_t blocks = std::min<uint32_t>(cdiv(n_union, kAbundThreads), 1024);
    hipLaunchKernelGGL(k_abund_delta, dim3(blocks), dim3(kAbundThreads), 0, s, n_union, reinterpret_cast<unsigned long long*>(mass),
                       reinterpret_cast<unsigned long long*>(next), reinterpret_cast<unsigned long long*>(l1));
}

void launch_abund_final(hipStream_t s, uint32_t blocks, const AbundEntries& en, const uint64_t* mass, const uint32_t* ent_e, const uint64_t* read_id,
                        const uint32_t* u_tax, void* out, uint32_t* assigned) {
    if (!en.n_reads || !blocks) return;
    hipLaunchKernelGGL(k_abund_final, dim3(blocks), dim3(kAbundThreads), 0, s, en, reinterpret_cast<const unsigned long long*>(mass), ent_e,
                       reinterpret_cast<const unsigned long long*>(read_id), u_tax, (uint32_t*)out, assigned);
}

}  // namespace mtsv
