// k_compact.hip -- keep the reads of a resident batch whose match flag is clear (or set) and write them, packed, into the
// resident input of another workspace: the step between a filter index and a database that share one device
// (the reference goes through a FASTQ file here: mtsv-partition.rs:56-93 writes the unmatched reads,
// a second mtsv-binner process parses them again).
//
// A lane per source read, 1024 reads per workgroup, so the 64 reads of a wavefront are the 64 bits of one flag word
// (bit 0 of the bitmap is the first read of the source's run: k_match.hip) and a lane's rank among the wavefront's
// survivors is a population count of the word below its own bit.  Two quantities are scanned over the reads -- survivors
// and their bases -- the bases with a wavefront prefix; across workgroups by tile sums:
//   k_compact_count  per tile: survivors, their bases; the longest survivor (one atomicMax per workgroup)
//   k_compact_sums   one workgroup: exclusive scan of the tile sums in place, the totals into the result block
//   (the host reads the result block -- 24 bytes -- and checks them against the destination's capacity)
//   k_compact_copy   per tile: the scan inside the tile again, offsets and read map of its survivors, then their bases
// The copy: a survivor's source and destination byte offsets differ by an arbitrary amount, so a 16-lane group moves a
// read as destination-aligned dwords, each put together from two aligned source dwords (v_alignbyte); only the up to three
// bytes before the first and after the last aligned destination dword of a read go singly.  Every destination byte is
// written once, by one lane; nothing is written behind a read's last base, so the room the search kernels may read past
// the end of the code buffer (never what it holds) is the allocation's, as after upload() + run().
#include <hip/hip_runtime.h>

#include "k_tile.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kCompactThreads = 1024;
constexpr uint32_t kCompactWaves = kCompactThreads / kWave;
constexpr uint32_t kCopyGroup = 16;  // lanes that move one read: 64 bytes per trip (reads of 150 bases: three trips)

// the lane's read r of n: *mask = the survivors of its wavefront's 64 reads (the same in every lane), its own start and
// length (0 for a lane past the batch)
__device__ inline bool compact_read(uint32_t r, uint32_t n, const unsigned long long* __restrict__ words,
                                    const uint32_t* __restrict__ off, uint32_t keep_matched, unsigned long long* mask,
                                    uint32_t* start, uint32_t* len) {
    const uint32_t lane = lane_id(), first = r - lane;  // a multiple of 64
    unsigned long long m = 0;
    *start = 0;
    *len = 0;
    if (first < n) {
        const unsigned long long w = words[first >> 6];
        const uint32_t left = n - first;
        m = (keep_matched ? w : ~w) & (left >= 64 ? ~0ull : (1ull << left) - 1ull);
    }
    if (r < n) {
        *start = off[r];
        *len = off[r + 1] - *start;
    }
    *mask = m;
    return (m >> lane) & 1ull;
}

// result: [0] survivors, [1] their bases (k_compact_sums), [2] the longest survivor (zeroed by the caller)
__global__ __launch_bounds__(kCompactThreads) void k_compact_count(uint32_t n, const unsigned long long* __restrict__ words,
                                                                   const uint32_t* __restrict__ off, uint32_t keep_matched,
                                                                   unsigned long long* __restrict__ tile_cnt,
                                                                   unsigned long long* __restrict__ tile_bases,
                                                                   unsigned long long* __restrict__ result) {
    __shared__ uint32_t s_cnt[kCompactWaves], s_len[kCompactWaves], s_max[kCompactWaves];
    const uint32_t r = blockIdx.x * kCompactThreads + threadIdx.x;
    unsigned long long mask;
    uint32_t start, len;
    const bool kept = compact_read(r, n, words, off, keep_matched, &mask, &start, &len);
    uint32_t sum = kept ? len : 0, mx = sum;
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_down(sum, d);
        mx = max(mx, (uint32_t)__shfl_down(mx, d));
    }
    if (lane_id() == 0) {
        s_cnt[threadIdx.x / kWave] = (uint32_t)__popcll(mask);
        s_len[threadIdx.x / kWave] = sum;
        s_max[threadIdx.x / kWave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long c = 0, b = 0;
        uint32_t m = 0;
        for (uint32_t w = 0; w < kCompactWaves; w++) {
            c += s_cnt[w];
            b += s_len[w];
            m = max(m, s_max[w]);
        }
        tile_cnt[blockIdx.x] = c;
        tile_bases[blockIdx.x] = b;
        if (m) atomicMax(result + 2, (unsigned long long)m);
    }
}

// one workgroup: both arrays of tile sums become exclusive prefixes, the totals go to result[0] and result[1]
__global__ __launch_bounds__(1024) void k_compact_sums(unsigned long long* __restrict__ tile_cnt,
                                                       unsigned long long* __restrict__ tile_bases, uint32_t n_tiles,
                                                       unsigned long long* __restrict__ result) {
    __shared__ unsigned long long buf[1024];
    __shared__ unsigned long long carry;
    for (int a = 0; a < 2; a++) {
        unsigned long long* t = a ? tile_bases : tile_cnt;
        if (threadIdx.x == 0) carry = 0;
        __syncthreads();
        for (uint32_t base = 0; base < n_tiles; base += 1024) {
            const uint32_t i = base + threadIdx.x;
            const unsigned long long v = i < n_tiles ? t[i] : 0;
            buf[threadIdx.x] = v;
            __syncthreads();
            for (int d = 1; d < 1024; d <<= 1) {
                const unsigned long long o = threadIdx.x >= (uint32_t)d ? buf[threadIdx.x - d] : 0;
                __syncthreads();
                buf[threadIdx.x] += o;
                __syncthreads();
            }
            const unsigned long long incl = buf[threadIdx.x], c = carry;
            if (i < n_tiles) t[i] = c + incl - v;
            __syncthreads();
            if (threadIdx.x == 1023) carry = c + incl;
            __syncthreads();
        }
        if (threadIdx.x == 0) result[a] = carry;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kCompactThreads) void k_compact_copy(uint32_t n, const unsigned long long* __restrict__ words,
                                                                  const uint32_t* __restrict__ off, const uint8_t* __restrict__ codes,
                                                                  uint32_t keep_matched, const uint32_t* __restrict__ src_map,
                                                                  const unsigned long long* __restrict__ tile_cnt,
                                                                  const unsigned long long* __restrict__ tile_bases,
                                                                  const unsigned long long* __restrict__ result,
                                                                  uint8_t* __restrict__ dst_codes, uint32_t* __restrict__ dst_off,
                                                                  uint32_t* __restrict__ dst_map) {
    __shared__ uint32_t s_cnt[kCompactWaves], s_len[kCompactWaves];
    __shared__ uint32_t s_src[kCompactThreads], s_dst[kCompactThreads], s_n[kCompactThreads];  // by rank inside the tile
    const uint32_t r = blockIdx.x * kCompactThreads + threadIdx.x, lane = lane_id(), wave = threadIdx.x / kWave;
    unsigned long long mask;
    uint32_t start, len;
    const bool kept = compact_read(r, n, words, off, keep_matched, &mask, &start, &len);
    const uint32_t mine = kept ? len : 0;
    const uint32_t incl = wave_incl_sum(mine);
    if (lane == kWave - 1) s_len[wave] = incl;
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), at = incl - mine, tile_n = 0;
    for (uint32_t w = 0; w < kCompactWaves; w++) {
        if (w < wave) {
            rank += s_cnt[w];
            at += s_len[w];
        }
        tile_n += s_cnt[w];
    }
    if (kept) {
        const uint32_t j = (uint32_t)tile_cnt[blockIdx.x] + rank, d = (uint32_t)tile_bases[blockIdx.x] + at;
        dst_off[j] = d;
        dst_map[j] = src_map ? src_map[r] : r;
        s_src[rank] = start;
        s_dst[rank] = d;
        s_n[rank] = len;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) dst_off[result[0]] = (uint32_t)result[1];  // the closing entry (the only one when nothing survives)
    __syncthreads();
    // ---- the tile's survivors, a 16-lane group per read, a read of any length in a loop ----
    const uint32_t l = threadIdx.x & (kCopyGroup - 1);
    for (uint32_t k = threadIdx.x / kCopyGroup; k < tile_n; k += kCompactThreads / kCopyGroup) {
        const uint32_t S = s_src[k], D = s_dst[k], L = s_n[k];
        const uint32_t head = min(L, (4u - (D & 3u)) & 3u);  // bytes before the first aligned destination dword
        const uint32_t body = (L - head) >> 2;               // whole destination dwords
        const uint32_t tail = L - head - 4 * body;           // bytes after the last
        if (l < head) dst_codes[D + l] = codes[S + l];
        if (l >= 4 && l - 4 < tail) {
            const uint32_t o = head + 4 * body + (l - 4);
            dst_codes[D + o] = codes[S + o];
        }
        const uint32_t sb = S + head, sh = sb & 3u;
        const uint32_t* __restrict__ s32 = reinterpret_cast<const uint32_t*>(codes) + (sb >> 2);
        uint32_t* __restrict__ d32 = reinterpret_cast<uint32_t*>(dst_codes) + ((D + head) >> 2);
        // (the second source dword of a read's last trip may lie up to four bytes behind the read: inside the buffer's slack)
        for (uint32_t i = l; i < body; i += kCopyGroup) d32[i] = __builtin_amdgcn_alignbyte(s32[i + 1], s32[i], sh);
    }
}

// the hits a pass of a compacted workspace has just gathered: resident read number -> the caller's
__global__ __launch_bounds__(256) void k_remap_reads(DevHit* __restrict__ hits, uint64_t n, const uint32_t* __restrict__ map) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hits[i].read = map[hits[i].read];
}

}  // namespace

uint32_t compact_tiles(uint64_t n_reads) { return std::max(1u, cdiv(n_reads, kCompactThreads)); }

void launch_compact_scan(hipStream_t s, uint32_t n_reads, const uint64_t* words, const uint32_t* read_off, int keep_matched, uint64_t* tile_cnt,
                         uint64_t* tile_bases, uint64_t* result) {
    const uint32_t tiles = compact_tiles(n_reads);
    hipLaunchKernelGGL(k_compact_count, dim3(tiles), dim3(kCompactThreads), 0, s, n_reads, reinterpret_cast<const unsigned long long*>(words), read_off,
                       (uint32_t)(keep_matched != 0), reinterpret_cast<unsigned long long*>(tile_cnt), reinterpret_cast<unsigned long long*>(tile_bases),
                       reinterpret_cast<unsigned long long*>(result));
    hipLaunchKernelGGL(k_compact_sums, dim3(1), dim3(1024), 0, s, reinterpret_cast<unsigned long long*>(tile_cnt),
                       reinterpret_cast<unsigned long long*>(tile_bases), tiles, reinterpret_cast<unsigned long long*>(result));
}

void launch_compact_copy(hipStream_t s, uint32_t n_reads, const uint64_t* words, const uint32_t* read_off, const uint8_t* codes, int keep_matched,
                         const uint32_t* src_map, const uint64_t* tile_cnt, const uint64_t* tile_bases, const uint64_t* result, uint8_t* dst_codes,
                         uint32_t* dst_off, uint32_t* dst_map) {
    hipLaunchKernelGGL(k_compact_copy, dim3(compact_tiles(n_reads)), dim3(kCompactThreads), 0, s, n_reads, reinterpret_cast<const unsigned long long*>(words),
                       read_off, codes, (uint32_t)(keep_matched != 0), src_map, reinterpret_cast<const unsigned long long*>(tile_cnt),
                       reinterpret_cast<const unsigned long long*>(tile_bases), reinterpret_cast<const unsigned long long*>(result), dst_codes, dst_off,
                       dst_map);
}

void launch_remap_reads(hipStream_t s, DevHit* hits, uint64_t n_hits, const uint32_t* map) {
    if (!n_hits) return;
    hipLaunchKernelGGL(k_remap_reads, dim3(cdiv(n_hits, 256)), dim3(256), 0, s, hits, n_hits, map);
}

}  // namespace mtsv
