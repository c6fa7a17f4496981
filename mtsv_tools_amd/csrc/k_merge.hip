// k_merge.hip -- the hit lists of several runs over the same reads (one run per chunk of a database cut with mtsv-chunk)
// merged per read into one list, in HBM: read by read the hits of the first source, then the second, and so on, every
// source in its own order -- the list mtsv_bin_batch_chunks puts together on the host (capi.cpp), left where k_report,
// k_match and the download can take it as if a pass had gathered it.
//
// A source's hits lie in PARTS (the segments of its run: a range of its reads each, hits ordered by `read`, in the
// caller's numbers when the batch is mapped -- the map ascends, so the order holds per resident read too).  Three kernels
// around the existing scan:
//   k_merge_bounds  a lane per (part, read of the part): where the read's hits begin in the part and how many there are
//                   -- two lower bounds over the `read` fields (keys k and k + 1), the second inside what the first left
//   k_merge_sum     a lane per read: its merged count (nout[2j], nout[2j + 1] = 0: a pass's layout) and, per source, what
//                   to add to a hit's position in its part to get its place behind out_off[2j]
//   (launch_scan over nout gives out_off)
//   k_merge_copy    a lane per SOURCE HIT: two 16-byte loads, its read's number (the `read` field, through the map by a
//                   binary search when mapped), two 16-byte stores
// No lane's work grows with a read's hit count: a read with thousands of hits is thousands of lanes of the copy.
#include <hip/hip_runtime.h>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kMergeThreads = 256;

// first i in [lo, hi) with hits[i].read >= key (hi when there is none)
__device__ inline uint32_t merge_lower(const DevHit* __restrict__ hits, uint32_t lo, uint32_t hi, uint64_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (hits[mid].read < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kMergeThreads) void k_merge_bounds(const MergePart* __restrict__ parts, uint32_t n_reads,
                                                                const uint32_t* __restrict__ map, uint32_t* __restrict__ lo_out,
                                                                uint32_t* __restrict__ cnt_out) {
    const MergePart p = parts[blockIdx.y];
    const uint32_t i = blockIdx.x * kMergeThreads + threadIdx.x;
    if (i >= p.n_reads) return;
    const uint32_t j = p.first_read + i;
    const uint64_t key = map ? (uint64_t)map[j] : (uint64_t)j;
    const uint32_t lo = merge_lower(p.hits, 0, p.count, key);
    const uint32_t hi = merge_lower(p.hits, lo, p.count, key + 1);
    const uint64_t at = (uint64_t)p.src * n_reads + j;
    lo_out[at] = lo;
    cnt_out[at] = hi - lo;
}

// cnt_base: in, the counts; out, per (source, read): (hits of the earlier sources for the read) - (the read's first
// position in its part), modulo 2^32 -- the copy adds a hit's position in its part
__global__ __launch_bounds__(kMergeThreads) void k_merge_sum(uint32_t n_reads, uint32_t n_srcs, const uint32_t* __restrict__ lo,
                                                             uint32_t* __restrict__ cnt_base, uint2* __restrict__ nout) {
    const uint32_t j = blockIdx.x * kMergeThreads + threadIdx.x;
    if (j >= n_reads) return;
    uint32_t acc = 0;
    for (uint32_t s = 0; s < n_srcs; s++) {
        const uint64_t at = (uint64_t)s * n_reads + j;
        const uint32_t c = cnt_base[at];
        cnt_base[at] = acc - lo[at];
        acc += c;
    }
    nout[j] = make_uint2(acc, 0u);
}

__global__ __launch_bounds__(kMergeThreads) void k_merge_copy(const MergePart* __restrict__ parts, uint32_t n_reads,
                                                              const uint32_t* __restrict__ map, const uint32_t* __restrict__ base,
                                                              const uint32_t* __restrict__ out_off, DevHit* __restrict__ dst,
                                                              uint32_t n_dst, unsigned long long* __restrict__ n_dropped) {
    const MergePart p = parts[blockIdx.y];
    const uint32_t i = blockIdx.x * kMergeThreads + threadIdx.x;
    if (i >= p.count) return;
    const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(p.hits + i);
    const uint4 a = s4[0], b = s4[1];
    const uint64_t read = (uint64_t)a.x | (uint64_t)a.y << 32;
    uint32_t j;
    if (map) {  // the resident read whose caller number this is, inside the part's range
        uint32_t lo = p.first_read, hi = p.first_read + p.n_reads;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((uint64_t)map[mid] < read) lo = mid + 1;
            else hi = mid;
        }
        j = lo;
    } else {
        j = (uint32_t)read;
    }
    // a hit without a read of its part, or a place outside the list: the sources' order is not what the bounds assumed.
    // Nothing is written for it; it is counted, and the host makes an error of a count that is not zero
    const bool no_read = read >> 32 || j < p.first_read || j - p.first_read >= p.n_reads || (map && (uint64_t)map[j] != read);
    const uint32_t d = no_read ? n_dst : out_off[2 * j] + base[(uint64_t)p.src * n_reads + j] + i;
    if (d >= n_dst) {
        atomicAdd(n_dropped, 1ull);
        return;
    }
    uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst + d);
    d4[0] = a;
    d4[1] = b;
}

}  // namespace

void launch_merge_bounds(hipStream_t s, const MergePart* parts, uint32_t n_parts, uint32_t max_part_reads, uint32_t n_reads,
                         const uint32_t* map, uint32_t* lo, uint32_t* cnt) {
    if (!n_parts || !max_part_reads) return;
    hipLaunchKernelGGL(k_merge_bounds, dim3(cdiv(max_part_reads, kMergeThreads), n_parts), dim3(kMergeThreads), 0, s, parts, n_reads, map, lo,
                       cnt);
}

void launch_merge_sum(hipStream_t s, uint32_t n_reads, uint32_t n_srcs, const uint32_t* lo, uint32_t* cnt_base, uint32_t* nout) {
    if (!n_reads) return;
    hipLaunchKernelGGL(k_merge_sum, dim3(cdiv(n_reads, kMergeThreads)), dim3(kMergeThreads), 0, s, n_reads, n_srcs, lo, cnt_base,
                       reinterpret_cast<uint2*>(nout));
}

void launch_merge_copy(hipStream_t s, const MergePart* parts, uint32_t n_parts, uint32_t max_part_hits, uint32_t n_reads,
                       const uint32_t* map, const uint32_t* base, const uint32_t* out_off, DevHit* dst, uint32_t n_dst, uint64_t* n_dropped) {
    if (!n_parts || !max_part_hits) return;
    hipLaunchKernelGGL(k_merge_copy, dim3(cdiv(max_part_hits, kMergeThreads), n_parts), dim3(kMergeThreads), 0, s, parts, n_reads, map, base,
                       out_off, dst, n_dst, reinterpret_cast<unsigned long long*>(n_dropped));
}

}  // namespace mtsv
