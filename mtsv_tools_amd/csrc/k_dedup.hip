// k_dedup.hip -- which reads of a resident batch are identical, and the records of a fold fanned out from one read of every
// group to the others: the two ends of binning a sequence once however often the batch holds it (dedup.hip; DESIGN.md
// section 7, "Identical reads").  The reference tree has no such step: the workflow around it collapses duplicates on the
// CPU before mtsv-binner and loses the reads' IDs.
//
// Two reads are identical when their lengths and all their codes (0..4, k_normalise has run) are equal.  rep(j) is the
// smallest index of a read identical to j -- whatever the hash does:
//   k_dedup_hash     a 16-lane group per read.  The read is taken as READ-RELATIVE dwords, each put together from two aligned
//                    dwords of the buffer (v_alignbyte), the last one masked to the read's bytes, so the hash is that of the
//                    codes and not of where they lie.  Every dword is mixed with its position, the sum of those (any order)
//                    with the length: 64 bits per read.
//   k_dedup_insert   an open-addressing table of 64-bit slots in HBM, empty = all ones, a slot = (tag : 32, read index : 32).
//                    A group probes linearly from its hash.  An empty slot is claimed with a compare-and-swap; at a slot with
//                    its tag the group compares lengths, then dwords, with the read the slot names -- any read that ever held
//                    a slot has the codes of every other, so the index may change underneath -- and on equality lowers the
//                    slot's index with a 64-bit atomic min (the tag, the upper half, is equal); otherwise the next slot.  A
//                    slot never becomes empty again and never changes its sequence, so the first slot on a chain that a read
//                    claims or finds equal is the same for every identical read.  Only the group's first lane touches the
//                    table and hands what it saw to the others: no lock, no lane waits for another.  The loop is bounded by
//                    the slot count; a read that runs out of slots raises the error counter.  The read's slot is kept.
//   k_dedup_resolve  a lane per read: rep from its slot, now final; the "is its own representative" bits of a wavefront are
//                    one ballot, one word of a bitmap laid out like the match flags (k_match.hip), which k_compact.hip packs
//                    the representatives by; read[j] and rep[j] in the caller's numbers; representatives counted.
//
// The fan (mtsv_fold_expand): entry j of the map takes the records the source list holds for read rep[j], `read` replaced
// by read[j].
//   k_fan_count      a lane per entry: lower and upper bound of rep[j] in the sorted records, the count; the records found
//                    for self-representing entries are summed (the host compares the sum with the list's length: a record
//                    of a read that represents nothing would be lost)
//   (launch_scan over the counts)
//   k_fan_write      OUTPUT-parallel, like k_fold: a workgroup owns `tile` output records, finds the entries of its first and
//                    last record by binary search in the scanned offsets, every record its entry between those two; then
//                    the tile is written dword by dword, consecutive lanes consecutive words.  A read with thousands of records
//                    and hundreds of copies costs what as many records spread evenly cost.
#include <hip/hip_runtime.h>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kDedupGroup = 16;    // lanes per read, as k_compact_copy's
constexpr uint32_t kDedupThreads = 256;  // 16 reads per workgroup
constexpr unsigned long long kDedupEmpty = ~0ull;

__device__ inline uint64_t dedup_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// value of `from` (the group's lane 0 .. 15) in every lane of the 16-lane group
__device__ inline uint32_t group_get(uint32_t v, int from) { return (uint32_t)__shfl((int)v, from, kDedupGroup); }
__device__ inline uint64_t group_get64(uint64_t v, int from) {
    return (uint64_t)group_get((uint32_t)v, from) | (uint64_t)group_get((uint32_t)(v >> 32), from) << 32;
}
__device__ inline uint32_t group_or(uint32_t v) {
    for (int d = 1; d < (int)kDedupGroup; d <<= 1) v |= (uint32_t)__shfl_xor((int)v, d, kDedupGroup);
    return v;
}
__device__ inline uint64_t group_sum64(uint64_t v) {
    for (int d = 1; d < (int)kDedupGroup; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, kDedupGroup), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, kDedupGroup);
        v += (uint64_t)lo | (uint64_t)hi << 32;
    }
    return v;
}

// read-relative dword i (< ceil(L / 4)) of the read of L codes at byte S, bytes behind the read zero.  The second aligned
// dword is loaded only when it holds a byte of the read: nothing is read behind the dword of the read's last code.
__device__ inline uint32_t dedup_dword(const uint8_t* __restrict__ codes, uint32_t S, uint32_t L, uint32_t i) {
    const uint32_t* __restrict__ s32 = reinterpret_cast<const uint32_t*>(codes) + (S >> 2) + i;
    const uint32_t sh = S & 3u;
    const uint32_t lo = s32[0];
    const uint32_t hi = (sh && 4u * i + 4u - sh < L) ? s32[1] : 0u;
    const uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, sh);
    const uint32_t valid = L - 4u * i;  // >= 1
    return valid >= 4u ? w : w & ((1u << (8u * valid)) - 1u);
}

__global__ __launch_bounds__(kDedupThreads) void k_dedup_hash(uint32_t n, const uint32_t* __restrict__ off, const uint8_t* __restrict__ codes,
                                                              unsigned long long* __restrict__ hash) {
    const uint32_t j = (blockIdx.x * kDedupThreads + threadIdx.x) / kDedupGroup, l = threadIdx.x & (kDedupGroup - 1);
    if (j >= n) return;  // (the whole group)
    const uint32_t S = off[j], L = off[j + 1] - S, nd = (L + 3u) >> 2;
    uint64_t h = 0;
    for (uint32_t i = l; i < nd; i += kDedupGroup) h += dedup_mix((uint64_t)dedup_dword(codes, S, L, i) | (uint64_t)(i + 1u) << 32);
    h = group_sum64(h);
    if (l == 0) hash[j] = dedup_mix(h ^ ((uint64_t)L * 0x9E3779B97F4A7C15ull));
}

// are reads a and b equal?  (the same answer in every lane of the group)
__device__ inline bool dedup_equal(const uint32_t* __restrict__ off, const uint8_t* __restrict__ codes, uint32_t Sa, uint32_t La, uint32_t b, uint32_t l) {
    const uint32_t Sb = off[b], Lb = off[b + 1] - Sb;
    if (La != Lb) return false;
    const uint32_t nd = (La + 3u) >> 2;
    for (uint32_t base = 0; base < nd; base += kDedupGroup) {
        const uint32_t i = base + l;
        const uint32_t diff = i < nd ? dedup_dword(codes, Sa, La, i) ^ dedup_dword(codes, Sb, Lb, i) : 0u;
        if (group_or(diff)) return false;
    }
    return true;
}

// ctr: [0] representatives (k_dedup_resolve), [1] reads without a slot
__global__ __launch_bounds__(kDedupThreads) void k_dedup_insert(uint32_t n, const uint32_t* __restrict__ off, const uint8_t* __restrict__ codes,
                                                                const unsigned long long* __restrict__ hash, uint64_t hash_mask,
                                                                unsigned long long* __restrict__ table, uint32_t slot_mask, uint32_t* __restrict__ slot_of,
                                                                unsigned long long* __restrict__ ctr) {
    const uint32_t j = (blockIdx.x * kDedupThreads + threadIdx.x) / kDedupGroup, l = threadIdx.x & (kDedupGroup - 1);
    if (j >= n) return;
    const uint32_t S = off[j], L = off[j + 1] - S;
    const uint64_t h = hash[j] & hash_mask;
    const uint32_t tag = (uint32_t)(h >> 32);
    const unsigned long long mine = (unsigned long long)tag << 32 | j;
    uint32_t s = (uint32_t)h & slot_mask, found = 0xffffffffu;
    for (uint32_t step = 0; step <= slot_mask; step++, s = (s + 1u) & slot_mask) {
        unsigned long long cur = 0;
        uint32_t claimed = 0;
        if (l == 0) {
            cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kDedupEmpty) {
                cur = atomicCAS(table + s, kDedupEmpty, mine);
                claimed = cur == kDedupEmpty;
            }
        }
        claimed = group_get(claimed, 0);
        if (claimed) {
            found = s;
            break;
        }
        cur = group_get64(cur, 0);
        if ((uint32_t)(cur >> 32) != tag) continue;
        if (!dedup_equal(off, codes, S, L, (uint32_t)cur, l)) continue;
        if (l == 0) atomicMin(table + s, mine);
        found = s;
        break;
    }
    if (l == 0) {
        slot_of[j] = found;
        if (found == 0xffffffffu) atomicAdd(ctr + 1, 1ull);
    }
}

__global__ __launch_bounds__(256) void k_dedup_resolve(uint32_t n, const unsigned long long* __restrict__ table, const uint32_t* __restrict__ slot_of,
                                                       const uint32_t* __restrict__ src_map, unsigned long long* __restrict__ words,
                                                       uint32_t* __restrict__ read, uint32_t* __restrict__ rep, unsigned long long* __restrict__ ctr) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;  // (a wavefront's 64 reads are one word: 256 is a multiple of 64)
    bool self = false;
    if (j < n) {
        const uint32_t s = slot_of[j];
        const uint32_t r = s == 0xffffffffu ? j : (uint32_t)table[s];  // (without a slot: the error is counted, the map stays in range)
        self = r == j;
        read[j] = src_map ? src_map[j] : j;
        rep[j] = src_map ? src_map[r] : r;
    }
    const unsigned long long b = __ballot(self);
    if (lane_id() == 0 && j < n) {
        words[j >> 6] = b;
        if (b) atomicAdd(ctr, (unsigned long long)__popcll(b));
    }
}

// ---- the fan ----
// the first record of rec[0 .. n) (W words each, ordered by the u64 `read` in words 0 and 1) whose read is >= key (upper: > key)
__device__ inline uint32_t fan_bound(const uint32_t* __restrict__ rec, uint32_t n, uint32_t W, uint64_t key, bool upper) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t* r = rec + (uint64_t)mid * W;
        const uint64_t v = (uint64_t)r[0] | (uint64_t)r[1] << 32;
        if (upper ? v <= key : v < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ctr: [0] the records found for self-representing entries
__global__ __launch_bounds__(256) void k_fan_count(uint32_t n, const uint32_t* __restrict__ read, const uint32_t* __restrict__ rep,
                                                   const uint32_t* __restrict__ rec, uint32_t n_rec, uint32_t W, uint32_t* __restrict__ first,
                                                   uint32_t* __restrict__ cnt, unsigned long long* __restrict__ ctr) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    uint32_t own = 0;
    if (j < n) {
        const uint32_t r = rep[j];
        const uint32_t lb = fan_bound(rec, n_rec, W, r, false), ub = fan_bound(rec, n_rec, W, r, true);
        first[j] = lb;
        cnt[j] = ub - lb;
        if (r == read[j]) own = ub - lb;
    }
    unsigned long long sum = own;
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d);
    if (lane_id() == 0 && sum) atomicAdd(ctr, sum);
}

// the last entry e of off[0 .. n] (ascending, off[n] = total > p) with off[e] <= p, searched in [lo, hi]
__device__ inline uint32_t fan_entry(const uint32_t* __restrict__ off, uint32_t lo, uint32_t hi, uint32_t p) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_fan_write(uint32_t n, const uint32_t* __restrict__ read, const uint32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ off, const uint32_t* __restrict__ rec, uint32_t W, uint32_t tile,
                                                   uint32_t total, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_src[kFanTileMax], s_read[kFanTileMax];
    __shared__ uint32_t s_e[2];
    const uint32_t p0 = blockIdx.x * tile;  // (tiles * tile < 2^32 + tile: the grid is cut from total < 2^32, p0 < total)
    const uint32_t cnt = min(tile, total - p0);
    if (threadIdx.x < 2) s_e[threadIdx.x] = fan_entry(off, 0, n - 1, threadIdx.x ? p0 + cnt - 1 : p0);
    __syncthreads();
    const uint32_t e0 = s_e[0], e1 = s_e[1];
    for (uint32_t k = threadIdx.x; k < cnt; k += 256) {
        const uint32_t e = fan_entry(off, e0, e1, p0 + k);
        s_src[k] = first[e] + (p0 + k - off[e]);
        s_read[k] = read[e];
    }
    __syncthreads();
    uint32_t* __restrict__ o = out + (uint64_t)p0 * W;
    for (uint32_t q = threadIdx.x; q < cnt * W; q += 256) {
        const uint32_t k = q / W, w = q - k * W;
        o[q] = w == 0 ? s_read[k] : w == 1 ? 0u : rec[(uint64_t)s_src[k] * W + w];
    }
}

}  // namespace

void launch_dedup_hash(hipStream_t s, uint32_t n_reads, const uint32_t* read_off, const uint8_t* codes, uint64_t* hash) {
    if (!n_reads) return;
    hipLaunchKernelGGL(k_dedup_hash, dim3(cdiv((uint64_t)n_reads * kDedupGroup, kDedupThreads)), dim3(kDedupThreads), 0, s, n_reads, read_off, codes,
                       reinterpret_cast<unsigned long long*>(hash));
}

void launch_dedup_insert(hipStream_t s, uint32_t n_reads, const uint32_t* read_off, const uint8_t* codes, const uint64_t* hash, uint32_t hash_bits,
                         uint64_t* table, uint32_t n_slots, uint32_t* slot_of, uint64_t* ctr) {
    if (!n_reads) return;
    const uint64_t hash_mask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1ull;
    hipLaunchKernelGGL(k_dedup_insert, dim3(cdiv((uint64_t)n_reads * kDedupGroup, kDedupThreads)), dim3(kDedupThreads), 0, s, n_reads, read_off, codes,
                       reinterpret_cast<const unsigned long long*>(hash), hash_mask, reinterpret_cast<unsigned long long*>(table), n_slots - 1, slot_of,
                       reinterpret_cast<unsigned long long*>(ctr));
}

void launch_dedup_resolve(hipStream_t s, uint32_t n_reads, const uint64_t* table, const uint32_t* slot_of, const uint32_t* src_map, uint64_t* words,
                          uint32_t* read, uint32_t* rep, uint64_t* ctr) {
    if (!n_reads) return;
    hipLaunchKernelGGL(k_dedup_resolve, dim3(cdiv(n_reads, 256)), dim3(256), 0, s, n_reads, reinterpret_cast<const unsigned long long*>(table), slot_of,
                       src_map, reinterpret_cast<unsigned long long*>(words), read, rep, reinterpret_cast<unsigned long long*>(ctr));
}

static uint32_t fan_words(int grain) { return grain == kCollapseGrainTaxid ? 4u : 6u; }

void launch_fan_count(hipStream_t s, int grain, uint32_t n_entries, const uint32_t* read, const uint32_t* rep, const void* rec, uint32_t n_rec,
                      uint32_t* first, uint32_t* cnt, uint64_t* ctr) {
    if (!n_entries) return;
    hipLaunchKernelGGL(k_fan_count, dim3(cdiv(n_entries, 256)), dim3(256), 0, s, n_entries, read, rep, static_cast<const uint32_t*>(rec), n_rec,
                       fan_words(grain), first, cnt, reinterpret_cast<unsigned long long*>(ctr));
}

void launch_fan_write(hipStream_t s, int grain, uint32_t n_entries, const uint32_t* read, const uint32_t* first, const uint32_t* off, const void* rec,
                      uint32_t tile, uint32_t total, void* out) {
    if (!n_entries || !total) return;
    hipLaunchKernelGGL(k_fan_write, dim3(cdiv(total, tile)), dim3(256), 0, s, n_entries, read, first, off, static_cast<const uint32_t*>(rec), fan_words(grain),
                       tile, total, static_cast<uint32_t*>(out));
}

}  // namespace mtsv
