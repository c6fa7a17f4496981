// k_place.hip -- the alignment of an accepted hit: where it lies in its reference and its edit script (place.hip,
// mtsv_batch_place_hits).
//
// A hit (read, strand, tax_id, gi, offset, edit) names a read, a strand of it and the start of a window in the bin of
// (tax_id, gi).  With P the read's codes on that strand (L of them), T the text from the window's start to the bin's end and
// D the semi-global matrix of align.rs:28-85 (D[0][j] = 0, D[i][0] = i, unit costs; an N matches nothing), the placement is
//   end    the smallest j with D[L][j] <= e, e = min(edit, L) (D[L][0] = L: an edit of L or more ends at column 0)
//   path   from (L, end) while i > 0: the diagonal when j > 0 and D[i-1][j-1] + (match ? 0 : 1) == D[i][j] ('=' or 'X'), else
//          the step up when D[i-1][j] + 1 == D[i][j] ('I'), else the step left ('D'); start = j where i reaches 0
// The path costs D[L][end] <= e, so it holds at most e ops that are not '=' and at most 2e + 1 runs, and it consumes at most
// L + e columns: it never leaves columns end - (L + e) .. end.
//
//   k_place_map  a lane per hit: its bin (a binary search over the index's (tax_id, gi) keys), its resident read (the hit's
//                number itself, or a lower bound in the ascending read map of a workspace filled by take_reads), e, and the
//                2e + 1 op slots it may need.  It writes scratch and counters only: the host refuses the call on the counters
//                (unknown reference, offset at or beyond the bin's length, read not resident, strand above 1) before anything
//                else runs, and sizes the ring by the largest L + e it reports.
//   (launch_scan over the slots: off[0 .. n], off[n] = the ops array's length)
//   k_place<W>   a lane per hit, W = myers_words(longest resident read) words per column, the hits strided by the whole grid.
//                Forward: the multi-word Myers/Hyyro column step in registers, the match masks from the read's bit planes
//                (built by the lane from the resident codes), the text in aligned 16-byte pieces.  After every column -- column 0
//                included -- the lane stores the column's vertical deltas (Pv, Mv) into its ring in HBM, laid out
//                [column mod R][Pv words, Mv words][lane of the grid]: the lanes of a wavefront advance column by column
//                together, so a store instruction writes 256 consecutive bytes.  The scan stops at the first column whose
//                last-row score is <= e, or at the bin's end (the hit is then UNPLACEABLE: counted, nothing written).
//                Backward: D[i][j] = popc(Pv_j & low(i)) - popc(Mv_j & low(i)); the lane keeps columns j and j - 1 in registers
//                (a step to the left loads one column from the ring), evaluates at most two cells a step beside the one it
//                stands on, and writes the runs backwards from the end of its slots, so that they read in reference order.
//                R is a power of two >= L + e + 2 for every hit: column j - 1 of the leftmost column the path can reach is
//                still in the ring.
// Every store is a plain vector store to memory the lane owns; the counters are integer adds, minima and maxima.
#include <hip/hip_runtime.h>

#include <string>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kPlaceThreads = 256;
constexpr uint32_t kPlaceNone = 0xffffffffu;

__global__ __launch_bounds__(kPlaceThreads) void k_place_map(const DevHit* __restrict__ hits, uint32_t n, const uint64_t* __restrict__ bin_key,
                                                            const uint32_t* __restrict__ bin_of_key, uint32_t n_keys, const DevBin* __restrict__ bins,
                                                            const uint32_t* __restrict__ read_off, uint32_t n_reads, const uint32_t* __restrict__ read_map,
                                                            uint32_t* __restrict__ hit_bin, uint32_t* __restrict__ hit_read, uint32_t* __restrict__ cnt,
                                                            unsigned long long* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlaceThreads + threadIdx.x;
    bool unknown = false, range = false, absent = false, strand = false;
    uint32_t span = 0;
    if (i < n) {
        const DevHit h = hits[i];
        const uint64_t key = (uint64_t)h.tax_id << 32 | h.gi;
        uint32_t lo = 0, hi = n_keys;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (bin_key[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        unknown = !(lo < n_keys && bin_key[lo] == key);
        uint32_t b = kPlaceNone, r = kPlaceNone;
        if (!unknown) {
            b = bin_of_key[lo];
            const DevBin bin = bins[b];
            range = h.offset >= (uint64_t)(bin.end - bin.start);
        }
        if (read_map) {  // the hit carries the caller's number: the resident read that maps to it
            uint32_t l = 0, u = n_reads;
            while (l < u) {
                const uint32_t mid = l + ((u - l) >> 1);
                if ((uint64_t)read_map[mid] < h.read) l = mid + 1;
                else u = mid;
            }
            if (l < n_reads && (uint64_t)read_map[l] == h.read) r = l;
        } else if (h.read < n_reads) {
            r = (uint32_t)h.read;
        }
        absent = r == kPlaceNone;
        strand = h.strand > 1;
        const bool bad = unknown || range || absent || strand;
        uint32_t slots = 0;
        if (!bad) {
            const uint32_t L = read_off[r + 1] - read_off[r];
            const uint32_t e = min(h.edit, L);
            slots = 2 * e + 1;
            span = L + e;
        }
        hit_bin[i] = bad ? kPlaceNone : b;
        hit_read[i] = bad ? kPlaceNone : r;
        cnt[i] = slots;
    }
    for (int d = kWave / 2; d > 0; d >>= 1) span = max(span, (uint32_t)__shfl_xor((int)span, d));
    const unsigned long long um = __ballot(unknown), rm = __ballot(range), am = __ballot(absent), sm = __ballot(strand), bad = um | rm | am | sm;
    if (lane_id() == 0) {
        if (um) atomicAdd(&ctr[kPlaceCtrUnknown], (unsigned long long)__popcll(um));
        if (rm) atomicAdd(&ctr[kPlaceCtrRange], (unsigned long long)__popcll(rm));
        if (am) atomicAdd(&ctr[kPlaceCtrAbsent], (unsigned long long)__popcll(am));
        if (sm) atomicAdd(&ctr[kPlaceCtrStrand], (unsigned long long)__popcll(sm));
        if (bad) atomicMin(&ctr[kPlaceCtrFirstBad], (unsigned long long)(i + (uint32_t)__builtin_ctzll(bad)));  // (lane 0 holds i of lane 0)
        if (span) atomicMax(&ctr[kPlaceCtrSpan], (unsigned long long)span);
    }
}

// D[i][j] from column j's vertical deltas: the sum of the first i of them
template <int W>
__device__ inline int place_cell(const uint32_t (&pv)[W], const uint32_t (&mv)[W], uint32_t i) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
        const uint32_t lo = 32u * w;
        const uint32_t m = i >= lo + 32 ? 0xffffffffu : (i > lo ? (1u << (i - lo)) - 1u : 0u);
        s += __popc(pv[w] & m) - __popc(mv[w] & m);
    }
    return s;
}

struct PlaceArgs {
    const DevHit* hits;
    uint32_t n;
    const uint32_t* hit_bin;
    const uint32_t* hit_read;
    const DevBin* bins;
    uint32_t n_bins;
    const uint8_t* text;
    const uint8_t* codes;
    const uint32_t* read_off;
    const uint32_t* off;   // the scan: hit i owns ops[off[i] .. off[i + 1])
    uint32_t* ring;        // (ring_mask + 1) columns x 2 W words x the grid's lanes
    uint32_t ring_mask;
    uint32_t* ops;
    uint32_t* out;         // 12 words per hit: mtsv_placement
    unsigned long long* ctr;
};

template <int W>
__global__ __launch_bounds__(kPlaceThreads) void k_place(PlaceArgs a) {
    const uint32_t tid = blockIdx.x * kPlaceThreads + threadIdx.x;
    const uint64_t T = (uint64_t)gridDim.x * kPlaceThreads;
    uint32_t* const ring = a.ring + tid;
    // column `col` of this lane: word w of Pv at [w * T], of Mv at [(W + w) * T]
    auto column = [&](uint32_t col) { return ring + (uint64_t)(col & a.ring_mask) * (2 * W) * T; };
    for (uint64_t i = tid; i < a.n; i += T) {
        const uint32_t bi = a.hit_bin[i], r = a.hit_read[i];
        if (bi >= a.n_bins || r == kPlaceNone) continue;  // (cannot be: the host launches after a map pass without a refusal)
        const DevHit h = a.hits[i];
        const DevBin bin = a.bins[bi];
        const uint32_t ro = a.read_off[r], L = a.read_off[r + 1] - ro;
        const uint32_t e = min(h.edit, L);
        const uint32_t t0 = bin.start + (uint32_t)h.offset, tlen = bin.end - t0;
        const uint8_t* const rd = a.codes + ro;
        const bool rev = h.strand != 0;
        if (L > 32u * W) continue;  // (cannot be: W is chosen for the longest resident read)
        // the strand's bit planes: bit 0 and bit 1 of the code, and "is a base" (an N matches nothing)
        uint32_t b0[W], b1[W], ok[W];
#pragma unroll
        for (int w = 0; w < W; w++) {
            uint32_t x0 = 0, x1 = 0, xk = 0;
            for (uint32_t q = 0; q < 32 && 32u * w + q < L; q++) {
                const uint32_t p = 32u * w + q;
                const uint32_t c = rev ? comp_code(rd[L - 1 - p]) : (uint32_t)rd[p];
                x0 |= (c & 1u) << q;
                x1 |= ((c >> 1) & 1u) << q;
                xk |= (c < 4 ? 1u : 0u) << q;
            }
            b0[w] = x0;
            b1[w] = x1;
            ok[w] = xk;
        }
        // ---- forward: column by column until the last row's score is within e ----
        uint32_t pv[W], mv[W];
#pragma unroll
        for (int w = 0; w < W; w++) {
            pv[w] = 0xffffffffu;
            mv[w] = 0;
        }
        {
            uint32_t* c = column(0);
#pragma unroll
            for (int w = 0; w < W; w++) {
                c[(uint64_t)w * T] = pv[w];
                c[(uint64_t)(W + w) * T] = mv[w];
            }
        }
        const uint32_t wl = L ? (L - 1) >> 5 : 0, bl = L ? (L - 1) & 31 : 0;
        int score = (int)L;
        uint32_t end = score <= (int)e ? 0u : kPlaceNone;
        uint4 piece = make_uint4(0, 0, 0, 0);
        for (uint32_t j = 1; end == kPlaceNone && j <= tlen; j++) {
            const uint32_t pos = t0 + j - 1, k = pos & 15u;
            // (the text array is padded to whole 64-byte sectors: an aligned piece that holds a position below n lies inside it)
            if (j == 1 || k == 0) piece = *reinterpret_cast<const uint4*>(a.text + (pos & ~15u));
            const uint32_t word = k < 4 ? piece.x : k < 8 ? piece.y : k < 12 ? piece.z : piece.w;
            const uint32_t t = (word >> (8 * (k & 3u))) & 0xffu;
            const uint32_t m0 = (t & 1u) ? 0u : 0xffffffffu, m1 = (t & 2u) ? 0u : 0xffffffffu, tk = t < 4 ? 0xffffffffu : 0u;
            int hin = 0;  // D[0][j] - D[0][j - 1]
#pragma unroll
            for (int w = 0; w < W; w++) {
                uint32_t eq = (b0[w] ^ m0) & (b1[w] ^ m1) & ok[w] & tk;
                const uint32_t neg = hin < 0 ? 1u : 0u;
                const uint32_t xv = eq | mv[w];
                eq |= neg;
                const uint32_t xh = (((eq & pv[w]) + pv[w]) ^ pv[w]) | eq;
                uint32_t ph = mv[w] | ~(xh | pv[w]);
                uint32_t mh = pv[w] & xh;
                if (w == (int)wl) score += (int)((ph >> bl) & 1u) - (int)((mh >> bl) & 1u);
                const int hout = (int)(ph >> 31) - (int)(mh >> 31);
                ph = (ph << 1) | (hin > 0 ? 1u : 0u);
                mh = (mh << 1) | neg;
                pv[w] = mh | ~(xv | ph);
                mv[w] = ph & xv;
                hin = hout;
            }
            uint32_t* c = column(j);
#pragma unroll
            for (int w = 0; w < W; w++) {
                c[(uint64_t)w * T] = pv[w];
                c[(uint64_t)(W + w) * T] = mv[w];
            }
            if (score <= (int)e) end = j;
        }
        if (end == kPlaceNone) {
            atomicAdd(&a.ctr[kPlaceCtrUnplaceable], 1ull);
            atomicMin(&a.ctr[kPlaceCtrFirstUnplaceable], (unsigned long long)i);
            continue;
        }
        // ---- backward: (pv, mv) is column `end`; (pl, ml) the column to its left ----
        uint32_t pl[W], ml[W];
        auto load_left = [&](uint32_t j) {  // column j - 1 into (pl, ml), j > 0
            const uint32_t* c = column(j - 1);
#pragma unroll
            for (int w = 0; w < W; w++) {
                pl[w] = c[(uint64_t)w * T];
                ml[w] = c[(uint64_t)(W + w) * T];
            }
        };
#pragma unroll
        for (int w = 0; w < W; w++) pl[w] = ml[w] = 0;
        uint32_t ri = L, j = end;
        if (j > 0) load_left(j);
        const uint32_t slot_lo = a.off[i], slot_hi = a.off[i + 1];
        uint32_t at = slot_hi, run_op = 0, run_len = 0;
        bool broken = false;
        int d = score;  // D[ri][j]
        while (ri > 0 && !broken) {
            uint32_t op = 0;
            bool moved_left = false;
            bool done = false;
            if (j > 0) {
                const uint32_t t = a.text[t0 + j - 1];
                const uint32_t c = rev ? comp_code(rd[L - ri]) : (uint32_t)rd[ri - 1];
                const bool match = c < 4 && c == t;
                const int dd = place_cell<W>(pl, ml, ri - 1);
                if (dd + (match ? 0 : 1) == d) {
                    op = match ? 7u : 8u;
                    ri--;
                    d = dd;
                    moved_left = true;
                    done = true;
                }
            }
            if (!done) {
                const int du = place_cell<W>(pv, mv, ri - 1);
                if (j == 0 || du + 1 == d) {
                    op = 1u;
                    ri--;
                    d = du;
                } else {
                    op = 2u;
                    d = place_cell<W>(pl, ml, ri);
                    moved_left = true;
                }
            }
            if (moved_left) {
                j--;
#pragma unroll
                for (int w = 0; w < W; w++) {
                    pv[w] = pl[w];
                    mv[w] = ml[w];
                }
                if (j > 0) {
                    if (end - (j - 1) > a.ring_mask) broken = true;  // (cannot be: the path stays within L + e columns of its end)
                    else load_left(j);
                }
            }
            if (op == run_op) {
                run_len++;
            } else {
                if (run_len) {
                    if (at > slot_lo) a.ops[--at] = run_len << 4 | run_op;
                    else broken = true;  // (cannot be: at most 2e + 1 runs)
                }
                run_op = op;
                run_len = 1;
            }
        }
        if (run_len && !broken) {
            if (at > slot_lo) a.ops[--at] = run_len << 4 | run_op;
            else broken = true;
        }
        if (broken) {
            atomicAdd(&a.ctr[kPlaceCtrBroken], 1ull);
            continue;
        }
        atomicAdd(&a.ctr[kPlaceCtrColumns], (unsigned long long)end + 1);
        uint4* o = reinterpret_cast<uint4*>(a.out + i * 12);
        o[0] = make_uint4((uint32_t)h.read, (uint32_t)(h.read >> 32), h.tax_id, h.gi);
        o[1] = make_uint4(h.edit, (uint32_t)h.strand, (uint32_t)h.offset + j, (uint32_t)h.offset + end);
        o[2] = make_uint4(slot_hi - at, 0u, at, 0u);
    }
}

template <int W>
void launch_place_w(hipStream_t s, uint32_t blocks, const PlaceArgs& a) {
    hipLaunchKernelGGL(k_place<W>, dim3(blocks), dim3(kPlaceThreads), 0, s, a);
}

}  // namespace

uint32_t place_threads() { return kPlaceThreads; }

void launch_place_map(hipStream_t s, const DevHit* hits, uint32_t n, const uint64_t* bin_key, const uint32_t* bin_of_key, uint32_t n_keys, const DevBin* bins,
                      const uint32_t* read_off, uint32_t n_reads, const uint32_t* read_map, uint32_t* hit_bin, uint32_t* hit_read, uint32_t* cnt,
                      uint64_t* ctr) {
    if (!n) return;
    hipLaunchKernelGGL(k_place_map, dim3(cdiv(n, kPlaceThreads)), dim3(kPlaceThreads), 0, s, hits, n, bin_key, bin_of_key, n_keys, bins, read_off, n_reads,
                       read_map, hit_bin, hit_read, cnt, reinterpret_cast<unsigned long long*>(ctr));
}

void launch_place(hipStream_t s, uint32_t words, uint32_t blocks, const DevHit* hits, uint32_t n, const uint32_t* hit_bin, const uint32_t* hit_read,
                  const DevBin* bins, uint32_t n_bins, const uint8_t* text, const uint8_t* codes, const uint32_t* read_off, const uint32_t* off,
                  uint32_t* ring, uint32_t ring_cols, uint32_t* ops, void* out, uint64_t* ctr) {
    if (words < 2 || words > 8) throw std::runtime_error("internal: placement of reads of " + std::to_string(words) + " words");
    if (!ring_cols || (ring_cols & (ring_cols - 1))) throw std::runtime_error("internal: placement ring of " + std::to_string(ring_cols) + " columns");
    if (!n || !blocks) return;
    const PlaceArgs a{hits, n, hit_bin, hit_read, bins, n_bins, text, codes, read_off, off, ring, ring_cols - 1, ops, (uint32_t*)out,
                      reinterpret_cast<unsigned long long*>(ctr)};
    switch (words) {
    case 2: launch_place_w<2>(s, blocks, a); break;
    case 3: launch_place_w<3>(s, blocks, a); break;
    case 4: launch_place_w<4>(s, blocks, a); break;
    case 5: launch_place_w<5>(s, blocks, a); break;
    case 6: launch_place_w<6>(s, blocks, a); break;
    case 7: launch_place_w<7>(s, blocks, a); break;
    default: launch_place_w<8>(s, blocks, a); break;
    }
}

}  // namespace mtsv
