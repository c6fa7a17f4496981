// k_fold.hip -- two sorted lists of assignment records merged into one, one record per key with the better value: what
// lets the result of a chunk's run outlive the chunk (fold.hip).  A list is what k_collapse writes -- 16-byte records
// ordered by (read, tax_id), or 24-byte ones by (read, tax_id, gi, offset) / (read, tax_id, gi), every field unsigned,
// keys distinct inside a list -- so a key occurs at most twice in the union: once in A, the accumulator, once in B, a run.
//
// A merge path, in two passes over the same tiles:
//   A workgroup owns `tile` positions of the merged sequence WITH its duplicates, [d0, d1).  Among equal keys the A
//   record comes first.  Two lanes find, by binary search on the diagonals d0 and d1, how many A records lie before each
//   (fold_split); the tile's A and B stretches go to LDS with 16-byte loads; every record finds its merged position by one
//   binary search in the other stretch (A: the B records below it, B: the A records not above it).
//   The rule for equal keys: THE A RECORD STAYS and takes the better value, THE B RECORD IS DROPPED.  The partner of an A
//   record is the first B record not below it -- in LDS, or, when that is past the tile's B stretch, B[b1] in global
//   memory; the partner of a B record is the last A record not above it -- in LDS, or A[a0 - 1].  So a pair that straddles
//   a tile edge (A the last position of one tile, B the first of the next) is decided from the same two records by both
//   tiles, and the record written does not depend on where the edge falls.
//   k_fold<G, false>  counts the tile's survivors                        (then launch_scan over the tiles' counts)
//   k_fold<G, true>   the same, then a scan of the survivor flags in LDS, and the survivors to out[tile_off + rank],
//                     position by position: consecutive lanes write consecutive records
// Records are read twice and written once, nothing is written behind the last survivor, and there is no atomic on the way.
//
// Two kernels over an accumulated list, a lane per record, both from the records alone (a HEAD is a record whose `read`
// differs from its predecessor's):
//   k_fold_flags   a head sets bit `read` of a bitmap and counts as a matched read; a head at or above n_reads is counted
//                  apart (the host makes an error of it)
//   k_fold_report  a head walks its read's records -- those of a TaxID are contiguous in every grain -- and adds the
//                  read to one counter per TaxID, the categories as k_report.hip defines them; global atomics; a TaxID that
//                  the list does not hold is counted apart (the host makes an error of it)
#include <hip/hip_runtime.h>

#include <string>

#include "k_tile.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kFoldThreads = 256;
constexpr uint32_t kFoldMisc = 16;  // u32 behind the tile's arrays in LDS: [0], [1] the splits, [4 ..] the wavefronts' sums

template <int G>
struct FoldRec {
    static constexpr uint32_t W = G == kCollapseGrainTaxid ? 4 : 6;  // u32 per record
    static constexpr uint32_t kEdit = G == kCollapseGrainTaxid ? 3 : 5;
};

struct FoldKey {
    uint64_t read, mid;
    uint32_t lo;
};
__device__ inline bool fold_less(const FoldKey& a, const FoldKey& b) {
    if (a.read != b.read) return a.read < b.read;
    if (a.mid != b.mid) return a.mid < b.mid;
    return a.lo < b.lo;
}
__device__ inline bool fold_equal(const FoldKey& a, const FoldKey& b) { return a.read == b.read && a.mid == b.mid && a.lo == b.lo; }

// the key of the record at r (LDS or global): TAXID (read, tax_id); LONG (read, tax_id, gi, offset); TAXID_GI (read, tax_id, gi)
template <int G>
__device__ inline FoldKey fold_key(const uint32_t* r) {
    FoldKey k;
    k.read = (uint64_t)r[0] | (uint64_t)r[1] << 32;
    if (G == kCollapseGrainTaxid) {
        k.mid = r[2];
        k.lo = 0;
    } else {
        k.mid = (uint64_t)r[2] << 32 | r[3];
        k.lo = G == kCollapseGrainLong ? r[4] : 0;
    }
    return k;
}

// r keeps the better of its value and q's: the smaller edit; TAXID_GI the smaller (edit, offset).  Only value words of r
// are written: other lanes read r's key meanwhile
template <int G>
__device__ inline void fold_take_better(uint32_t* r, const uint32_t* q) {
    if (G == kCollapseGrainTaxidGi) {
        const uint32_t qe = q[5], qo = q[4];
        if (qe < r[5] || (qe == r[5] && qo < r[4])) {
            r[5] = qe;
            r[4] = qo;
        }
    } else {
        const uint32_t qe = q[FoldRec<G>::kEdit];
        if (qe < r[FoldRec<G>::kEdit]) r[FoldRec<G>::kEdit] = qe;
    }
}

// how many A records lie among the first d of the merged sequence (A first among equal keys)
template <int G>
__device__ inline uint32_t fold_split(const uint32_t* __restrict__ A, uint32_t n_a, const uint32_t* __restrict__ B, uint32_t n_b, uint64_t d) {
    constexpr uint32_t W = FoldRec<G>::W;
    uint32_t lo = d > n_b ? (uint32_t)(d - n_b) : 0, hi = (uint32_t)min(d, (uint64_t)n_a);
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        // (lo <= mid < hi: d - 1 - mid is in [0, n_b))
        const FoldKey ka = fold_key<G>(A + (uint64_t)mid * W), kb = fold_key<G>(B + (d - 1 - mid) * W);
        if (!fold_less(kb, ka)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// words [w0, w0 + nw) of g to dst[0 .. nw): 16-byte global loads from the first 16-byte boundary on (g itself is aligned so);
// the LDS side is four 4-byte stores per load (dst + head is 4-byte aligned only, in general)
__device__ inline void fold_load(uint32_t* dst, const uint32_t* __restrict__ g, uint64_t w0, uint32_t nw) {
    const uint32_t head = min((uint32_t)((4 - (w0 & 3)) & 3), nw);
    for (uint32_t i = threadIdx.x; i < head; i += kFoldThreads) dst[i] = g[w0 + i];
    const uint32_t nq = (nw - head) >> 2;
    const uint4* __restrict__ g4 = reinterpret_cast<const uint4*>(g + w0 + head);
    for (uint32_t q = threadIdx.x; q < nq; q += kFoldThreads) {
        const uint4 v = g4[q];
        uint32_t* d = dst + head + 4 * q;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    for (uint32_t i = head + 4 * nq + threadIdx.x; i < nw; i += kFoldThreads) dst[i] = g[w0 + i];
}

constexpr uint32_t kFoldDropped = 0xffffffffu;

template <int G, bool WRITE>
__global__ __launch_bounds__(kFoldThreads) void k_fold(const uint32_t* __restrict__ A, uint32_t n_a, const uint32_t* __restrict__ B, uint32_t n_b,
                                                       uint32_t tile, uint32_t* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_off,
                                                       uint32_t* __restrict__ out) {
    constexpr uint32_t W = FoldRec<G>::W;
    extern __shared__ __attribute__((aligned(16))) uint32_t fold_lds[];
    uint32_t* rec = fold_lds;         // the tile's A records, then its B records
    uint32_t* perm = rec + tile * W;  // merged position -> record of the tile
    uint32_t* flag = perm + tile;     // merged position -> survives; then its rank among the tile's survivors
    uint32_t* misc = flag + tile;
    const uint64_t n = (uint64_t)n_a + n_b;
    const uint64_t d0 = (uint64_t)blockIdx.x * tile, d1 = min(d0 + tile, n);
    if (threadIdx.x < 2) misc[threadIdx.x] = fold_split<G>(A, n_a, B, n_b, threadIdx.x ? d1 : d0);
    __syncthreads();
    // (sorted lists give a0 <= a1 <= a0 + (d1 - d0); the clamp keeps the stretches inside the tile's LDS whatever they hold)
    const uint32_t a0 = misc[0], a1 = min(max(misc[1], a0), a0 + (uint32_t)(d1 - d0));
    const uint32_t b0 = (uint32_t)(d0 - a0), b1 = (uint32_t)(d1 - a1);
    const uint32_t na = a1 - a0, nb = b1 - b0, nt = na + nb;
    uint32_t* recB = rec + na * W;
    fold_load(rec, A, (uint64_t)a0 * W, na * W);
    fold_load(recB, B, (uint64_t)b0 * W, nb * W);
    // (sorted lists with distinct keys give every position exactly one record; zeroed so that lists that are not cannot
    //  leave a position undefined)
    for (uint32_t p = threadIdx.x; p < nt; p += kFoldThreads) perm[p] = flag[p] = 0;
    __syncthreads();

    for (uint32_t e = threadIdx.x; e < nt; e += kFoldThreads) {
        if (e < na) {
            uint32_t* r = rec + e * W;
            const FoldKey k = fold_key<G>(r);
            uint32_t lo = 0, hi = nb;  // the B records of the tile below k
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (fold_less(fold_key<G>(recB + mid * W), k)) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t p = e + lo;
            flag[p] = 1;
            if (WRITE) {
                perm[p] = e;
                // the partner: the first B record not below k, which may be the first of the next tile
                const uint32_t* q = lo < nb ? recB + lo * W : b1 < n_b ? B + (uint64_t)b1 * W : nullptr;
                if (q && fold_equal(fold_key<G>(q), k)) fold_take_better<G>(r, q);
            }
        } else {
            const uint32_t j = e - na;
            const FoldKey k = fold_key<G>(recB + j * W);
            uint32_t lo = 0, hi = na;  // the A records of the tile not above k
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (!fold_less(k, fold_key<G>(rec + mid * W))) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t p = j + lo;
            // the partner: the last A record not above k, which may be the last of the tile before
            const uint32_t* q = lo ? rec + (lo - 1) * W : a0 ? A + (uint64_t)(a0 - 1) * W : nullptr;
            flag[p] = !(q && fold_equal(fold_key<G>(q), k));
            if (WRITE) perm[p] = e;
        }
    }
    __syncthreads();

    // the survivors before every position: a stretch of positions per lane, the lanes' sums by block_excl_sum
    const uint32_t ipt = (tile + kFoldThreads - 1) / kFoldThreads;
    const uint32_t p0 = min(threadIdx.x * ipt, nt), p1 = min(p0 + ipt, nt);
    uint32_t mine = 0;
    for (uint32_t p = p0; p < p1; p++) mine += flag[p];
    const BlockSum sum = block_excl_sum<kFoldThreads>(mine, misc + 4);
    if (!WRITE) {
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = sum.total;
        return;
    }
    uint32_t before = sum.before;
    for (uint32_t p = p0; p < p1; p++) {
        const uint32_t f = flag[p];
        flag[p] = f ? before : kFoldDropped;
        before += f;
    }
    __syncthreads();
    // (a tile writes inside the stretch the count pass gave it, whatever the lists hold)
    const uint64_t base = tile_off[blockIdx.x], end = tile_off[blockIdx.x + 1];
    for (uint32_t p = threadIdx.x; p < nt; p += kFoldThreads) {
        const uint32_t rank = flag[p];
        if (rank == kFoldDropped) continue;
        const uint32_t* r = rec + perm[p] * W;
        const uint64_t o = base + rank;
        if (o >= end) continue;
        uint32_t* dst = out + o * W;
        if (W == 4) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(r[0], r[1], r[2], r[3]);
        } else if (!(o & 1)) {  // (24-byte records: every other one begins on a 16-byte boundary)
            *reinterpret_cast<uint4*>(dst) = make_uint4(r[0], r[1], r[2], r[3]);
            *reinterpret_cast<uint2*>(dst + 4) = make_uint2(r[4], r[5]);
        } else {
            *reinterpret_cast<uint2*>(dst) = make_uint2(r[0], r[1]);
            *reinterpret_cast<uint4*>(dst + 2) = make_uint4(r[2], r[3], r[4], r[5]);
        }
    }
}

template <uint32_t W>
__global__ __launch_bounds__(kFoldThreads) void k_fold_flags(const uint32_t* __restrict__ rec, uint32_t n, uint64_t n_reads,
                                                             unsigned long long* __restrict__ words, unsigned long long* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * kFoldThreads + threadIdx.x;
    bool head = false, beyond = false;
    if (i < n) {
        const uint64_t read = rec_read_of<W>(rec, i);
        head = i == 0 || rec_read_of<W>(rec, i - 1) != read;
        beyond = head && read >= n_reads;
        head = head && !beyond;
        // (other heads of the wavefront may share the word)
        if (head) atomicOr(&words[read >> 6], 1ull << (read & 63));
    }
    const unsigned long long hm = __ballot(head), bm = __ballot(beyond);
    if (lane_id() == 0) {
        if (hm) atomicAdd(&ctr[0], (unsigned long long)__popcll(hm));
        if (bm) atomicAdd(&ctr[1], (unsigned long long)__popcll(bm));
    }
}

// counts: 4 per taxon (only_hit, only_best, tied_best, not_best), then the reads with a record, then the (read, TaxID) pairs
// whose TaxID is not in the list (none, unless the caller's list is incomplete: the host makes an error of them)
template <uint32_t W>
__global__ __launch_bounds__(kFoldThreads) void k_fold_report(const uint32_t* __restrict__ rec, uint32_t n, const uint32_t* __restrict__ taxa,
                                                              uint32_t n_taxa, unsigned long long* __restrict__ counts) {
    constexpr uint32_t kEdit = W - 1;
    const uint64_t i = (uint64_t)blockIdx.x * kFoldThreads + threadIdx.x;
    bool head = false;
    if (i < n) {
        const uint64_t read = rec_read_of<W>(rec, i);
        head = i == 0 || rec_read_of<W>(rec, i - 1) != read;
        if (head) {
            // first walk: the read's smallest edit m, its distinct TaxIDs, and how many of them are at m
            uint64_t end = i;
            uint32_t m = 0xffffffffu, nd = 0, best = 0, cur = 0, cur_min = 0;
            for (; end < n && rec_read_of<W>(rec, end) == read; end++) {
                const uint32_t t = rec[end * W + 2], e = rec[end * W + kEdit];
                if (end == i || t != cur) {
                    if (end != i) {
                        if (cur_min < m) m = cur_min, best = 1;
                        else if (cur_min == m) best++;
                    }
                    cur = t;
                    cur_min = e;
                    nd++;
                } else {
                    cur_min = min(cur_min, e);
                }
            }
            if (cur_min < m) m = cur_min, best = 1;
            else if (cur_min == m) best++;
            // second walk: every TaxID to its category
            for (uint64_t j = i; j < end;) {
                const uint32_t t = rec[j * W + 2];
                uint32_t e = rec[j * W + kEdit];
                for (j++; j < end && rec[j * W + 2] == t; j++) e = min(e, rec[j * W + kEdit]);
                const uint32_t cat = nd == 1 ? 0u : e != m ? 3u : best == 1 ? 1u : 2u;
                const uint32_t slot = find_u32(taxa, n_taxa, t);
                atomicAdd(slot < n_taxa ? &counts[4ull * slot + cat] : &counts[4ull * n_taxa + 1], 1ull);
            }
        }
    }
    const unsigned long long hm = __ballot(head);
    if (lane_id() == 0 && hm) atomicAdd(&counts[4ull * n_taxa], (unsigned long long)__popcll(hm));
}

uint32_t fold_lds_bytes(int grain, uint32_t tile) {
    const uint32_t w = grain == kCollapseGrainTaxid ? 4 : 6;
    return (tile * (w + 2) + kFoldMisc) * sizeof(uint32_t);
}

void fold_check(int grain, uint32_t n_a, uint32_t n_b, uint32_t tile) {
    if (grain != kCollapseGrainTaxid && grain != kCollapseGrainTaxidGi && grain != kCollapseGrainLong)
        throw std::runtime_error("internal: fold of grain " + std::to_string(grain));
    if (tile < 2 || tile > kFoldTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: fold tile of " + std::to_string(tile) + " positions");
    if ((uint64_t)n_a + n_b >= (1ull << 32)) throw std::runtime_error("internal: fold of 2^32 records or more");
}

}  // namespace

uint32_t fold_tiles(uint64_t n, uint32_t tile) { return cdiv(n, tile); }

void launch_fold_count(hipStream_t s, int grain, const void* a, uint32_t n_a, const void* b, uint32_t n_b, uint32_t tile, uint32_t* tile_cnt) {
    fold_check(grain, n_a, n_b, tile);
    const uint32_t tiles = fold_tiles((uint64_t)n_a + n_b, tile);
    if (!tiles) return;
    const uint32_t *A = (const uint32_t*)a, *B = (const uint32_t*)b;
    const uint32_t lds = fold_lds_bytes(grain, tile);
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL((k_fold<kCollapseGrainTaxid, false>), dim3(tiles), dim3(kFoldThreads), lds, s, A, n_a, B, n_b, tile, tile_cnt, nullptr, nullptr);
    else if (grain == kCollapseGrainLong)
        hipLaunchKernelGGL((k_fold<kCollapseGrainLong, false>), dim3(tiles), dim3(kFoldThreads), lds, s, A, n_a, B, n_b, tile, tile_cnt, nullptr, nullptr);
    else
        hipLaunchKernelGGL((k_fold<kCollapseGrainTaxidGi, false>), dim3(tiles), dim3(kFoldThreads), lds, s, A, n_a, B, n_b, tile, tile_cnt, nullptr, nullptr);
}

void launch_fold_write(hipStream_t s, int grain, const void* a, uint32_t n_a, const void* b, uint32_t n_b, uint32_t tile, const uint32_t* tile_off,
                       void* out) {
    fold_check(grain, n_a, n_b, tile);
    const uint32_t tiles = fold_tiles((uint64_t)n_a + n_b, tile);
    if (!tiles) return;
    const uint32_t *A = (const uint32_t*)a, *B = (const uint32_t*)b;
    uint32_t* o = (uint32_t*)out;
    const uint32_t lds = fold_lds_bytes(grain, tile);
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL((k_fold<kCollapseGrainTaxid, true>), dim3(tiles), dim3(kFoldThreads), lds, s, A, n_a, B, n_b, tile, nullptr, tile_off, o);
    else if (grain == kCollapseGrainLong)
        hipLaunchKernelGGL((k_fold<kCollapseGrainLong, true>), dim3(tiles), dim3(kFoldThreads), lds, s, A, n_a, B, n_b, tile, nullptr, tile_off, o);
    else
        hipLaunchKernelGGL((k_fold<kCollapseGrainTaxidGi, true>), dim3(tiles), dim3(kFoldThreads), lds, s, A, n_a, B, n_b, tile, nullptr, tile_off, o);
}

void launch_fold_flags(hipStream_t s, int grain, const void* rec, uint32_t n, uint64_t n_reads, uint64_t* words, uint64_t* ctr) {
    if (!n) return;
    auto* w = reinterpret_cast<unsigned long long*>(words);
    auto* c = reinterpret_cast<unsigned long long*>(ctr);
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL(k_fold_flags<4>, dim3(cdiv(n, kFoldThreads)), dim3(kFoldThreads), 0, s, (const uint32_t*)rec, n, n_reads, w, c);
    else
        hipLaunchKernelGGL(k_fold_flags<6>, dim3(cdiv(n, kFoldThreads)), dim3(kFoldThreads), 0, s, (const uint32_t*)rec, n, n_reads, w, c);
}

void launch_fold_report(hipStream_t s, int grain, const void* rec, uint32_t n, const uint32_t* taxa, uint32_t n_taxa, uint64_t* counts) {
    if (!n) return;
    auto* c = reinterpret_cast<unsigned long long*>(counts);
    if (grain == kCollapseGrainTaxid)
        hipLaunchKernelGGL(k_fold_report<4>, dim3(cdiv(n, kFoldThreads)), dim3(kFoldThreads), 0, s, (const uint32_t*)rec, n, taxa, n_taxa, c);
    else
        hipLaunchKernelGGL(k_fold_report<6>, dim3(cdiv(n, kFoldThreads)), dim3(kFoldThreads), 0, s, (const uint32_t*)rec, n, taxa, n_taxa, c);
}

}  // namespace mtsv
