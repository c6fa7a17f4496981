// k_text.hip -- the result lines of a sorted list of assignment records, written in HBM (text.hip): READ_ID:TAXID=EDIT,...
// from 16-byte records, READ_ID:TAXID-GI-OFFSET=EDIT,... from 24-byte ones, byte for byte what mtsv_format_assignments /
// mtsv_format_assignments_gi (capi.cpp) make of the same records and IDs on the host.
//
// Record-parallel: a record is the HEAD of its read when it is first in the list or its predecessor's `read` differs, and
// its bytes are
//   (a head only) its read's ID -- strnlen within the slot ids[id_off[read] .. id_off[read + 1]) -- and ':'
//   its fields, every number unsigned decimal with no padding
//   ',' or, when the next record belongs to another read or there is none, '\n'
// so the text is the concatenation of the records' bytes and a read with thousands of records costs what thousands of
// reads with one record do.  A workgroup owns `tile` consecutive records.  Three steps:
//   k_text_measure  rec_len[i] = the bytes of record i (digit counts by comparison with the powers of ten), tile_cnt[t] =
//                   their sum over tile t (u32: an ID slot is at most kTextIdMax bytes).  Counted apart, for the host to
//                   make an error of: heads whose read is at or above n_reads, heads whose ID slot does not lie inside the
//                   ID bytes (id_off not ascending) or is longer than kTextIdMax
//   k_text_scan_*   tile_off[t] = the byte at which tile t's text begins, 64 bits (the text of 2^32 records does not fit 32)
//   k_text_write    the tile's text is put together in LDS and stored.  The LDS image is a WINDOW of `cap` bytes of the
//                   output that begins on a 16-byte boundary of it; a tile whose text is longer takes several windows in
//                   turn.  Per window: every record whose bytes reach into it writes them (its lane: fields, separators,
//                   an ID of up to kTextLaneId bytes; a longer ID is put on a list and copied by the whole workgroup,
//                   consecutive lanes consecutive bytes); then the window leaves as 16-byte stores.  A tile's text begins
//                   and ends at arbitrary bytes, so the 16 bytes around an edge are shared with the neighbouring tile: of
//                   those each tile stores its own bytes, as dwords where a dword is its own and as single bytes where it
//                   is not.  No workgroup writes a byte outside [tile_off[t], tile_off[t + 1]), none is written twice, and
//                   nothing is read back.
#include <hip/hip_runtime.h>

#include <string>

#include "k_tile.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kTextThreads = 256;
constexpr uint32_t kTextLaneId = 64;  // an ID of up to this many bytes is copied by its record's lane, a longer one by the workgroup
constexpr uint32_t kTextMisc = 16;    // u32 behind the tile's arrays in LDS: [0] the length of the list, [4 ..] the wavefronts' sums
constexpr uint32_t kTextScanPer = 8, kTextScanChunk = kTextThreads * kTextScanPer;

// the decimal digits of v: the place of its highest bit gives floor(log10 v) or one more (1233 / 4096 is log10 2 from above),
// and one comparison with that power of ten decides
__device__ __constant__ uint32_t kTextPow10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};
__device__ inline uint32_t text_digits(uint32_t v) {
    v |= 1u;
    const uint32_t t = ((32u - (uint32_t)__clz((int)v)) * 1233u) >> 12;
    return t + 1u - (v < kTextPow10[t]);
}

// the bytes of a record's fields: "TAXID=EDIT" or "TAXID-GI-OFFSET=EDIT"
template <uint32_t W>
__device__ inline uint32_t text_item_bytes(const uint32_t* __restrict__ r) {
    if (W == 4) return text_digits(r[2]) + 1 + text_digits(r[3]);
    return text_digits(r[2]) + 1 + text_digits(r[3]) + 1 + text_digits(r[4]) + 1 + text_digits(r[5]);
}

template <uint32_t W>
__device__ inline uint64_t text_read_of(const uint32_t* __restrict__ rec, uint64_t i) {
    const uint32_t* r = rec + i * W;
    return (uint64_t)r[0] | (uint64_t)r[1] << 32;
}

// strnlen(ids + o0, o1 - o0): dword loads between the 4-byte boundaries of ids (which is aligned so), bytes around them
__device__ inline uint32_t text_strnlen(const uint8_t* __restrict__ ids, uint64_t o0, uint64_t o1) {
    uint64_t p = o0;
    for (; p < o1 && (p & 3); p++)
        if (!ids[p]) return (uint32_t)(p - o0);
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(ids);
    for (; p + 4 <= o1; p += 4) {
        const uint32_t v = w[p >> 2];
        if ((v - 0x01010101u) & ~v & 0x80808080u) {  // a zero byte among the four; the lowest address is the lowest byte
            uint32_t k = 0;
            while ((v >> (8 * k)) & 0xffu) k++;
            return (uint32_t)(p + k - o0);
        }
    }
    for (; p < o1; p++)
        if (!ids[p]) return (uint32_t)(p - o0);
    return (uint32_t)(o1 - o0);
}

template <uint32_t W>
__global__ __launch_bounds__(kTextThreads) void k_text_measure(const uint32_t* __restrict__ rec, uint32_t n, const uint8_t* __restrict__ ids,
                                                               const uint64_t* __restrict__ id_off, uint64_t n_reads, uint64_t ids_bytes, uint32_t tile,
                                                               uint32_t* __restrict__ rec_len, uint32_t* __restrict__ tile_cnt,
                                                               unsigned long long* __restrict__ ctr) {
    __shared__ uint32_t wave_sum[kTextThreads / kWave];
    const uint64_t g0 = (uint64_t)blockIdx.x * tile;
    const uint32_t nt = (uint32_t)min((uint64_t)tile, (uint64_t)n - g0);
    uint32_t mine = 0, bad_read = 0, bad_id = 0;
    for (uint32_t p = threadIdx.x; p < nt; p += kTextThreads) {
        const uint64_t g = g0 + p;
        const uint32_t* r = rec + g * W;
        const uint64_t read = (uint64_t)r[0] | (uint64_t)r[1] << 32;
        uint32_t b = text_item_bytes<W>(r) + 1;
        if (g == 0 || text_read_of<W>(rec, g - 1) != read) {
            if (read >= n_reads) {
                bad_read++;
            } else {
                const uint64_t o0 = id_off[read], o1 = id_off[read + 1];
                if (o0 > o1 || o1 > ids_bytes || o1 - o0 > kTextIdMax) bad_id++;
                else b += text_strnlen(ids, o0, o1) + 1;
            }
        }
        rec_len[g] = b;
        mine += b;
    }
    if (bad_read) atomicAdd(&ctr[0], (unsigned long long)bad_read);
    if (bad_id) atomicAdd(&ctr[1], (unsigned long long)bad_id);
    for (int d = kWave / 2; d; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d);
    if (lane_id() == 0) wave_sum[threadIdx.x / kWave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (uint32_t w = 0; w < kTextThreads / kWave; w++) total += wave_sum[w];
        tile_cnt[blockIdx.x] = total;
    }
}

// the sum of v over the lanes below this one (exclusive), and over the whole workgroup in *total
__device__ inline uint64_t text_block_scan(uint64_t v, uint64_t* sh, uint64_t* total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kTextThreads; d <<= 1) {
        const uint64_t t = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    const uint64_t incl = sh[threadIdx.x];
    *total = sh[kTextThreads - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kTextThreads) void k_text_scan_sums(const uint32_t* __restrict__ in, uint32_t n, uint64_t* __restrict__ sums) {
    __shared__ uint64_t sh[kTextThreads];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTextScanChunk + (uint64_t)threadIdx.x * kTextScanPer;
    uint64_t mine = 0, total;
    for (uint32_t k = 0; k < kTextScanPer; k++)
        if (i0 + k < n) mine += in[i0 + k];
    text_block_scan(mine, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. nb) become their exclusive prefix sums, *total their sum (one workgroup)
__global__ __launch_bounds__(kTextThreads) void k_text_scan_top(uint64_t* __restrict__ sums, uint32_t nb, uint64_t* __restrict__ total_out) {
    __shared__ uint64_t sh[kTextThreads];
    const uint32_t per = (nb + kTextThreads - 1) / kTextThreads;
    const uint32_t b0 = min(threadIdx.x * per, nb), b1 = min(b0 + per, nb);
    uint64_t mine = 0, total;
    for (uint32_t b = b0; b < b1; b++) mine += sums[b];
    uint64_t before = text_block_scan(mine, sh, &total);
    for (uint32_t b = b0; b < b1; b++) {
        const uint64_t v = sums[b];
        sums[b] = before;
        before += v;
    }
    if (threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(kTextThreads) void k_text_scan_apply(const uint32_t* __restrict__ in, uint32_t n, const uint64_t* __restrict__ sums,
                                                                  const uint64_t* __restrict__ total_in, uint64_t* __restrict__ out) {
    __shared__ uint64_t sh[kTextThreads];
    const uint64_t i0 = (uint64_t)blockIdx.x * kTextScanChunk + (uint64_t)threadIdx.x * kTextScanPer;
    uint32_t v[kTextScanPer];
    uint64_t mine = 0, total;
    for (uint32_t k = 0; k < kTextScanPer; k++) {
        v[k] = i0 + k < n ? in[i0 + k] : 0;
        mine += v[k];
    }
    uint64_t at = sums[blockIdx.x] + text_block_scan(mine, sh, &total);
    for (uint32_t k = 0; k < kTextScanPer; k++) {
        if (i0 + k < n) out[i0 + k] = at;
        at += v[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = *total_in;
}

// the window [lo, hi) of the tile's image coordinates lies in img[0 .. hi - lo)
struct TextWindow {
    uint8_t* img;
    uint32_t lo, hi;
    __device__ inline void put(uint32_t c, uint8_t ch) const {
        if (c >= lo && c < hi) img[c - lo] = ch;
    }
    __device__ inline uint32_t put_number(uint32_t c, uint32_t v) const {
        const uint32_t nd = text_digits(v);
        for (uint32_t k = nd; k--;) {
            put(c + k, (uint8_t)('0' + v % 10u));
            v /= 10u;
        }
        return c + nd;
    }
};

template <uint32_t W>
__global__ __launch_bounds__(kTextThreads) void k_text_write(const uint32_t* __restrict__ rec, uint32_t n, const uint8_t* __restrict__ ids,
                                                             const uint64_t* __restrict__ id_off, uint32_t tile, uint32_t cap,
                                                             const uint32_t* __restrict__ rec_len, const uint64_t* __restrict__ tile_off,
                                                             uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t text_lds[];
    uint8_t* img = text_lds;                                  // cap bytes of the output, from a 16-byte boundary of it
    uint32_t* off = reinterpret_cast<uint32_t*>(img + cap);  // tile + 1: where a record's bytes begin inside the tile's text
    uint32_t* list = off + tile + 1;                          // tile: the records whose ID the workgroup copies
    uint32_t* misc = list + tile;
    const uint64_t g0 = (uint64_t)blockIdx.x * tile;
    const uint32_t nt = (uint32_t)min((uint64_t)tile, (uint64_t)n - g0);
    const uint64_t B = tile_off[blockIdx.x], E = tile_off[blockIdx.x + 1];
    if (E <= B) return;
    // (the measure pass bounds a tile's text below 2^31 bytes)
    const uint32_t T = (uint32_t)min(E - B, (uint64_t)0x7fffffffu);

    // ---- the records' offsets: a stretch of positions per lane, the lanes' sums by block_excl_sum ----
    for (uint32_t p = threadIdx.x; p < nt; p += kTextThreads) off[p] = rec_len[g0 + p];
    __syncthreads();
    const uint32_t ipt = (tile + kTextThreads - 1) / kTextThreads;
    const uint32_t p0 = min(threadIdx.x * ipt, nt), p1 = min(p0 + ipt, nt);
    uint32_t mine = 0;
    for (uint32_t p = p0; p < p1; p++) mine += off[p];
    const BlockSum sum = block_excl_sum<kTextThreads>(mine, misc + 4);
    uint32_t before = sum.before;
    for (uint32_t p = p0; p < p1; p++) {
        const uint32_t v = off[p];
        off[p] = before;
        before += v;
    }
    if (threadIdx.x == 0) off[nt] = sum.total;
    __syncthreads();

    // image coordinate c of the tile is byte G0 + c of the output; the tile's text is [shift, shift + T)
    const uint64_t G0 = B & ~15ull;
    const uint32_t shift = (uint32_t)(B - G0);
    const uint32_t n_win = (shift + T + cap - 1) / cap;
    for (uint32_t w = 0; w < n_win; w++) {
        TextWindow win{img, w * cap, w * cap + cap};
        if (threadIdx.x == 0) misc[0] = 0;
        __syncthreads();
        // ---- every record that reaches into the window: its bytes, by its lane ----
        for (uint32_t p = threadIdx.x; p < nt; p += kTextThreads) {
            const uint32_t s = off[p] + shift, e = off[p + 1] + shift;
            if (e <= win.lo || s >= win.hi) continue;
            const uint64_t g = g0 + p;
            const uint32_t* r = rec + g * W;
            const uint64_t read = (uint64_t)r[0] | (uint64_t)r[1] << 32;
            const uint32_t item = text_item_bytes<W>(r);
            uint32_t c = s;
            if (g == 0 || text_read_of<W>(rec, g - 1) != read) {
                const uint32_t id_len = e - s >= item + 2 ? e - s - item - 2 : 0;
                if (id_len <= kTextLaneId) {
                    const uint8_t* id = ids + id_off[read];
                    for (uint32_t k = 0; k < id_len; k++) win.put(c + k, id[k]);
                } else {
                    list[atomicAdd(&misc[0], 1u)] = p;
                }
                c += id_len;
                win.put(c++, ':');
            }
            c = win.put_number(c, r[2]);
            if (W == 6) {
                win.put(c++, '-');
                c = win.put_number(c, r[3]);
                win.put(c++, '-');
                c = win.put_number(c, r[4]);
            }
            win.put(c++, '=');
            c = win.put_number(c, r[W - 1]);
            win.put(c, g + 1 == n || text_read_of<W>(rec, g + 1) != read ? '\n' : ',');
        }
        __syncthreads();
        // ---- the long IDs that reach into the window: consecutive lanes, consecutive bytes ----
        const uint32_t n_list = min(misc[0], nt);
        for (uint32_t j = 0; j < n_list; j++) {
            const uint32_t p = list[j];
            const uint32_t* r = rec + (g0 + p) * W;
            const uint64_t read = (uint64_t)r[0] | (uint64_t)r[1] << 32;
            const uint32_t s = off[p] + shift, e = off[p + 1] + shift, item = text_item_bytes<W>(r);
            const uint32_t id_len = e - s >= item + 2 ? e - s - item - 2 : 0;
            const uint8_t* id = ids + id_off[read];
            const uint32_t a = max(s, win.lo), b = min(s + id_len, win.hi);
            for (uint32_t c = a + threadIdx.x; c < b; c += kTextThreads) img[c - win.lo] = id[c - s];
        }
        __syncthreads();
        // ---- the window leaves: [a, b) of it is the tile's ----
        const uint32_t a = max(shift, win.lo) - win.lo, b = min(shift + T, win.hi) - win.lo;
        uint8_t* dst = out + G0 + (uint64_t)w * cap;
        for (uint32_t q = threadIdx.x; q * 16 < b; q += kTextThreads) {
            const uint32_t qa = q * 16;
            if (qa + 16 <= a) continue;
            if (qa >= a && qa + 16 <= b) {
                *reinterpret_cast<uint4*>(dst + qa) = *reinterpret_cast<const uint4*>(img + qa);
                continue;
            }
            // (an edge of the tile: the other bytes of these 16 are a neighbour's)
            for (uint32_t da = qa; da < qa + 16; da += 4) {
                if (da >= a && da + 4 <= b) {
                    *reinterpret_cast<uint32_t*>(dst + da) = *reinterpret_cast<const uint32_t*>(img + da);
                } else {
                    for (uint32_t k = da; k < da + 4; k++)
                        if (k >= a && k < b) dst[k] = img[k];
                }
            }
        }
        __syncthreads();
    }
}

void text_check(int grain, uint32_t tile) {
    if (grain != kCollapseGrainTaxid && grain != kCollapseGrainTaxidGi && grain != kCollapseGrainLong)
        throw std::runtime_error("internal: text of grain " + std::to_string(grain));
    if (tile < 2 || tile > kTextTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: text tile of " + std::to_string(tile) + " records");
}

}  // namespace

uint32_t text_tiles(uint64_t n, uint32_t tile) { return cdiv(n, tile); }
uint32_t text_scan_blocks(uint32_t tiles) { return cdiv(tiles ? tiles : 1, kTextScanChunk); }
uint32_t text_window_bytes(uint32_t tile) { return std::min<uint32_t>(std::max<uint32_t>(tile * 32, 256), 32768); }

void launch_text_measure(hipStream_t s, int grain, const void* rec, uint32_t n, const uint8_t* ids, const uint64_t* id_off, uint64_t n_reads,
                         uint64_t ids_bytes, uint32_t tile, uint32_t* rec_len, uint32_t* tile_cnt, uint64_t* ctr) {
    text_check(grain, tile);
    const uint32_t tiles = text_tiles(n, tile);
    if (!tiles) return;
    auto* c = reinterpret_cast<unsigned long long*>(ctr);
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL(k_text_measure<4>, dim3(tiles), dim3(kTextThreads), 0, s, (const uint32_t*)rec, n, ids, id_off, n_reads, ids_bytes, tile, rec_len,
                           tile_cnt, c);
    else
        hipLaunchKernelGGL(k_text_measure<6>, dim3(tiles), dim3(kTextThreads), 0, s, (const uint32_t*)rec, n, ids, id_off, n_reads, ids_bytes, tile, rec_len,
                           tile_cnt, c);
}

void launch_text_scan(hipStream_t s, const uint32_t* tile_cnt, uint32_t tiles, uint64_t* sums, uint64_t* total, uint64_t* tile_off) {
    if (!tiles) return;
    const uint32_t nb = text_scan_blocks(tiles);
    hipLaunchKernelGGL(k_text_scan_sums, dim3(nb), dim3(kTextThreads), 0, s, tile_cnt, tiles, sums);
    hipLaunchKernelGGL(k_text_scan_top, dim3(1), dim3(kTextThreads), 0, s, sums, nb, total);
    hipLaunchKernelGGL(k_text_scan_apply, dim3(nb), dim3(kTextThreads), 0, s, tile_cnt, tiles, sums, total, tile_off);
}

void launch_text_write(hipStream_t s, int grain, const void* rec, uint32_t n, const uint8_t* ids, const uint64_t* id_off, uint32_t tile,
                       const uint32_t* rec_len, const uint64_t* tile_off, uint8_t* out) {
    text_check(grain, tile);
    const uint32_t tiles = text_tiles(n, tile);
    if (!tiles) return;
    const uint32_t cap = text_window_bytes(tile);
    const uint32_t lds = cap + (2 * tile + 1 + kTextMisc) * sizeof(uint32_t);
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL(k_text_write<4>, dim3(tiles), dim3(kTextThreads), lds, s, (const uint32_t*)rec, n, ids, id_off, tile, cap, rec_len, tile_off, out);
    else
        hipLaunchKernelGGL(k_text_write<6>, dim3(tiles), dim3(kTextThreads), lds, s, (const uint32_t*)rec, n, ids, id_off, tile, cap, rec_len, tile_off, out);
}

}  // namespace mtsv
