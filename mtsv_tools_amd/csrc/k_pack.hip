// k_pack.hip -- the index file's raw bytes packed into the HBM layout (dev_layout.hpp) on the device: what upload_index does
// on host threads before its first copy, for MTSV_DEV_PACK_ON_DEVICE.  The bytes written are the host path's.
//
// Count / scan / write over the same tiles, as k_fold and k_text do it.  A workgroup owns a tile of T rank blocks (a power
// of two, 1 .. kPackTileMax; 128 rows each); a wavefront takes 64 rows at a time, a lane per row, and the three bit planes of
// those rows are three __ballot words.  Rows at and beyond n hold code 7, like the host's padding.
//   k_pack_count      per tile the A, C, G, T it holds; the sentinels and the bytes outside ACGTN$ (counted, with the row of
//                     the last sentinel and of the first foreign byte: the only atomics of the pack, with the Occ check's)
//   k_pack_scan       the tiles' counts to their exclusive prefixes, four u32 sequences at once, one workgroup
//   k_pack_blocks     per tile: planes and counts of its half blocks to LDS, a wavefront scan of the blocks' counts, then the
//                     blocks leave as 16-byte stores -- lane t writes quarter t & 3 of block t >> 2, so four consecutive lanes
//                     write one aligned 64-byte block and no block is written twice
//   k_pack_check_occ  a lane per Occ checkpoint j of the file: its six inclusive counts in bwt[0 ..= j * k] against
//                     block_rank(a, j * k + 1) on the blocks just written (N derived as every kernel derives it, '$' from the
//                     sentinel's row); a mismatch is counted and the smallest j kept
//   k_pack_text       text bytes to codes, 16 bytes per lane; the padding behind n is 7
// 1 byte read and 0.5 written per BWT symbol, 1 + 1 per text symbol; vector stores only.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kPackThreads = 256;
constexpr uint32_t kPackWaves = kPackThreads / 64;
constexpr uint32_t kPackScanThreads = 1024;

// dev_index.hip's sym_code
__device__ inline uint32_t pack_code(uint32_t c) {
    return c == 'A' ? kCodeA : c == 'C' ? kCodeC : c == 'G' ? kCodeG : c == 'T' ? kCodeT : c == 'N' ? kCodeN : c == '$' ? kCodeSentinel : 7u;
}

struct Planes {
    uint64_t m0, m1, m2;
};
// the planes of rows [row0, row0 + 64), row0 wave-uniform; *foreign: the rows below n whose byte is outside ACGTN$
__device__ inline Planes pack_planes(const uint8_t* __restrict__ bwt, uint64_t row0, uint32_t n, uint64_t* foreign) {
    const uint64_t row = row0 + lane_id();
    uint32_t code = 7;
    if (row < n) code = pack_code(bwt[row]);
    Planes p;
    p.m0 = __ballot(code & 1);
    p.m1 = __ballot(code & 2);
    p.m2 = __ballot(code & 4);
    if (foreign) *foreign = __ballot(row < n && code == 7);
    return p;
}
__device__ inline uint4 planes_acgt(const Planes& p) {
    return make_uint4(__popcll(~p.m0 & ~p.m1 & ~p.m2), __popcll(p.m0 & ~p.m1 & ~p.m2), __popcll(~p.m0 & p.m1 & ~p.m2),
                      __popcll(p.m0 & p.m1 & ~p.m2));
}
__device__ inline uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ inline uint4 sub4(uint4 a, uint4 b) { return make_uint4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ inline uint4 shfl_up4(uint4 v, uint32_t d) {
    return make_uint4(__shfl_up(v.x, d), __shfl_up(v.y, d), __shfl_up(v.z, d), __shfl_up(v.w, d));
}
// inclusive scan over the wavefront's lanes
__device__ inline uint4 wave_scan4(uint4 v) {
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint4 t = shfl_up4(v, d);
        if (lane_id() >= d) v = add4(v, t);
    }
    return v;
}

__global__ __launch_bounds__(kPackThreads) void k_pack_count(const uint8_t* __restrict__ bwt, uint32_t n, uint32_t n_blocks, uint32_t T,
                                                            uint4* __restrict__ tile_cnt, uint32_t* __restrict__ ctr) {
    __shared__ uint4 wsum[kPackWaves];
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t blk0 = (uint64_t)blockIdx.x * T;
    const uint32_t halves = 2 * (uint32_t)min((uint64_t)T, n_blocks - blk0);
    uint4 acc = make_uint4(0, 0, 0, 0);
    for (uint32_t h = wave; h < halves; h += kPackWaves) {
        const uint64_t row0 = (blk0 << kBlockShift) + 64ull * h;
        uint64_t foreign;
        const Planes p = pack_planes(bwt, row0, n, &foreign);
        acc = add4(acc, planes_acgt(p));
        const uint64_t sent = p.m0 & ~p.m1 & p.m2 & ~foreign;  // code 5 (7 has bit 1 set: padding never counts)
        if (lane_id() == 0) {
            if (foreign) {
                atomicAdd(&ctr[kPackCtrForeign], (uint32_t)__popcll(foreign));
                atomicMin(&ctr[kPackCtrForeignRow], (uint32_t)(row0 + (uint32_t)__ffsll((unsigned long long)foreign) - 1));
            }
            if (sent) {
                atomicAdd(&ctr[kPackCtrSentinels], (uint32_t)__popcll(sent));
                atomicMax(&ctr[kPackCtrSentinelRow], (uint32_t)(row0 + 63 - (uint32_t)__clzll((long long)sent)));
            }
        }
    }
    if (lane_id() == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = add4(add4(wsum[0], wsum[1]), add4(wsum[2], wsum[3]));
}

// tile[i] = sum of tile[0 .. i), in place; one workgroup walks the tiles kPackScanThreads at a time
__global__ __launch_bounds__(kPackScanThreads) void k_pack_scan(uint4* __restrict__ tile, uint32_t n_tiles) {
    __shared__ uint4 wsum[kPackScanThreads / 64];
    const uint32_t wave = threadIdx.x >> 6;
    uint4 carry = make_uint4(0, 0, 0, 0);
    for (uint32_t base = 0; base < n_tiles; base += kPackScanThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint4 v = i < n_tiles ? tile[i] : make_uint4(0, 0, 0, 0);
        const uint4 inc = wave_scan4(v);
        if (lane_id() == 63) wsum[wave] = inc;
        __syncthreads();
        uint4 before = carry;
        for (uint32_t w = 0; w < kPackScanThreads / 64; w++) {
            if (w == wave) before = add4(before, sub4(inc, v));
            if (w < wave) before = add4(before, wsum[w]);
            carry = add4(carry, wsum[w]);
        }
        if (i < n_tiles) tile[i] = before;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kPackThreads) void k_pack_blocks(const uint8_t* __restrict__ bwt, uint32_t n, uint32_t n_blocks, uint32_t T,
                                                             const uint4* __restrict__ tile_off, RankBlock* __restrict__ blocks) {
    __shared__ uint64_t plane[2 * kPackTileMax][3];  // per half block
    __shared__ uint4 hcnt[2 * kPackTileMax];
    __shared__ uint4 bpre[kPackTileMax];             // per block: the A, C, G, T of the tile's earlier blocks
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t blk0 = (uint64_t)blockIdx.x * T;
    const uint32_t tb = (uint32_t)min((uint64_t)T, n_blocks - blk0);  // blocks of this tile
    for (uint32_t h = wave; h < 2 * tb; h += kPackWaves) {
        const Planes p = pack_planes(bwt, (blk0 << kBlockShift) + 64ull * h, n, nullptr);
        if (lane_id() == 0) {
            plane[h][0] = p.m0;
            plane[h][1] = p.m1;
            plane[h][2] = p.m2;
            hcnt[h] = planes_acgt(p);
        }
    }
    __syncthreads();
    if (wave == 0) {
        const uint32_t b = lane_id();
        const uint4 own = b < tb ? add4(hcnt[2 * b], hcnt[2 * b + 1]) : make_uint4(0, 0, 0, 0);
        const uint4 inc = wave_scan4(own);
        if (b < tb) bpre[b] = sub4(inc, own);
    }
    __syncthreads();
    const uint32_t b = threadIdx.x >> 2, q = threadIdx.x & 3;
    if (b >= tb) return;
    uint4 v;
    if (q == 0) {
        v = add4(tile_off[blockIdx.x], bpre[b]);
    } else {
        const uint64_t lo = plane[2 * b][q - 1], hi = plane[2 * b + 1][q - 1];
        v = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    reinterpret_cast<uint4*>(blocks + blk0 + b)[q] = v;
}

__global__ __launch_bounds__(kPackThreads) void k_pack_check_occ(const RankBlock* __restrict__ blocks, uint32_t n, uint32_t k, uint32_t n_chk,
                                                                const uint64_t* __restrict__ occ, uint32_t* __restrict__ ctr) {
    const uint64_t j = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    const uint64_t i = j * k;
    if (j >= n_chk || i >= n) return;
    const uint32_t sentinel_row = ctr[kPackCtrSentinels] ? ctr[kPackCtrSentinelRow] : 0xffffffffu;
    const uint32_t pos = (uint32_t)i + 1, blk = pos >> kBlockShift, off = pos & (kBlockRows - 1);  // pos <= n: block n >> 7 exists
    const LoadedBlock b = load_block(blocks, blk);
    bool ok = occ[5ull * n_chk + j] == (sentinel_row <= i ? 1u : 0u);
    for (uint32_t a = 0; a < 5; a++) ok = ok && occ[(uint64_t)a * n_chk + j] == block_rank(b, a, blk, off, sentinel_row);
    if (!ok) {
        atomicAdd(&ctr[kPackCtrOccBad], 1u);
        atomicMin(&ctr[kPackCtrOccBadFirst], (uint32_t)j);
    }
}

__global__ __launch_bounds__(kPackThreads) void k_pack_text(const uint4* __restrict__ text, uint32_t n, uint64_t out_vecs, uint4* __restrict__ codes) {
    const uint64_t q = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (q >= out_vecs) return;
    const uint64_t at = q * 16;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (at < n) v = text[q];  // (the raw buffer is allocated in whole 16-byte vectors)
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t x = 0; x < 4; x++) {
        uint32_t o = 0;
#pragma unroll
        for (uint32_t y = 0; y < 4; y++) {
            const uint32_t code = at + 4 * x + y < n ? pack_code((w[x] >> (8 * y)) & 0xff) : 7u;
            o |= code << (8 * y);
        }
        w[x] = o;
    }
    codes[q] = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

uint32_t pack_tiles(uint32_t n_blocks, uint32_t tile) { return cdiv(n_blocks, tile); }

static void pack_check(uint32_t tile) {
    if (tile < 1 || tile > kPackTileMax || (tile & (tile - 1))) throw std::runtime_error("arg: pack tile must be a power of two, 1 .. 64 blocks");
}

void launch_pack_count(hipStream_t s, const uint8_t* bwt, uint32_t n, uint32_t n_blocks, uint32_t tile, uint4* tile_cnt, uint32_t* ctr) {
    pack_check(tile);
    hipLaunchKernelGGL(k_pack_count, dim3(pack_tiles(n_blocks, tile)), dim3(kPackThreads), 0, s, bwt, n, n_blocks, tile, tile_cnt, ctr);
}

void launch_pack_scan(hipStream_t s, uint4* tile_cnt, uint32_t n_tiles) {
    hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(kPackScanThreads), 0, s, tile_cnt, n_tiles);
}

void launch_pack_blocks(hipStream_t s, const uint8_t* bwt, uint32_t n, uint32_t n_blocks, uint32_t tile, const uint4* tile_off, RankBlock* blocks) {
    pack_check(tile);
    hipLaunchKernelGGL(k_pack_blocks, dim3(pack_tiles(n_blocks, tile)), dim3(kPackThreads), 0, s, bwt, n, n_blocks, tile, tile_off, blocks);
}

void launch_pack_check_occ(hipStream_t s, const RankBlock* blocks, uint32_t n, uint32_t k, uint32_t n_chk, const uint64_t* occ, uint32_t* ctr) {
    if (!n_chk) return;
    hipLaunchKernelGGL(k_pack_check_occ, dim3(cdiv(n_chk, kPackThreads)), dim3(kPackThreads), 0, s, blocks, n, k, n_chk, occ, ctr);
}

void launch_pack_text(hipStream_t s, const uint8_t* text, uint32_t n, uint8_t* codes, uint64_t codes_bytes) {
    const uint64_t vecs = codes_bytes / 16;
    hipLaunchKernelGGL(k_pack_text, dim3(cdiv(vecs, kPackThreads)), dim3(kPackThreads), 0, s, (const uint4*)text, n, vecs, (uint4*)codes);
}

}  // namespace mtsv
