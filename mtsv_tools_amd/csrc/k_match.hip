// k_match.hip -- one flag bit per read of a pass: did the run return a hit for it, on either strand
// (mtsv-partition.rs:34-54: the set of read IDs the reference's tool collects from the results text, here as a bitmap
// over the call's reads, from k_resolve's per-strand hit counts while they are in HBM).
//
// A lane per read; one __ballot per wavefront gives the flags of 64 consecutive reads.  The bitmap is indexed by the
// read's number in the whole call, and a pass starts wherever the one before it ended, so a wavefront's 64 flags
// straddle two 64-bit words as a rule; the lanes of a host batch run their passes on streams of their own at the same
// time, so the word a pass ends in may be the word another lane's pass begins in.  Hence: the (up to) two parts of a
// wavefront's mask go to their words with an atomicOr each -- parts that are zero are skipped, the bitmap was zeroed
// when the run began.  The matched reads are counted along the way: the wavefronts of a workgroup add their
// population counts in LDS, the workgroup adds the sum to the one global counter once.
#include <hip/hip_runtime.h>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kMatchThreads = 1024;  // 16 wavefronts: one add on the global counter per 1024 reads

__global__ __launch_bounds__(kMatchThreads) void k_match(uint32_t n_reads, const uint2* __restrict__ strand_nout, uint64_t first_bit,
                                                         unsigned long long* __restrict__ words,
                                                         unsigned long long* __restrict__ n_matched) {
    __shared__ uint32_t s_matched;
    if (threadIdx.x == 0) s_matched = 0;
    __syncthreads();
    const uint32_t r = blockIdx.x * kMatchThreads + threadIdx.x;
    bool hit = false;
    if (r < n_reads) {
        const uint2 n = strand_nout[r];  // (forward, reverse complement)
        hit = (n.x + n.y) != 0;
    }
    const unsigned long long m = __ballot(hit);
    const uint32_t lane = lane_id();
    if (m) {  // (the same for every lane of the wavefront)
        // bit of the wavefront's first read; its flags are bits [sh, 64) of word w and bits [0, sh) of word w + 1.  A
        // non-zero upper part belongs to a read of this pass, so word w + 1 is inside the bitmap.
        const uint64_t b0 = first_bit + (r - lane);
        const uint64_t w = b0 >> 6;
        const uint32_t sh = (uint32_t)(b0 & 63);
        const unsigned long long lo = m << sh, hi = sh ? m >> (64 - sh) : 0ull;
        if (lane == 0 && lo) atomicOr(&words[w], lo);
        if (lane == 1 && hi) atomicOr(&words[w + 1], hi);
        if (lane == 2) atomicAdd(&s_matched, (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_matched) atomicAdd(n_matched, (unsigned long long)s_matched);
}

}  // namespace

void launch_match(hipStream_t s, uint32_t n_reads, const uint32_t* strand_nout, uint64_t first_bit, uint64_t* words, uint64_t* n_matched) {
    if (!n_reads) return;
    hipLaunchKernelGGL(k_match, dim3(cdiv(n_reads, kMatchThreads)), dim3(kMatchThreads), 0, s, n_reads,
                       reinterpret_cast<const uint2*>(strand_nout), first_bit, reinterpret_cast<unsigned long long*>(words),
                       reinterpret_cast<unsigned long long*>(n_matched));
}

}  // namespace mtsv
