// k_cover.hip -- coverage per reference sequence from the records of a fold at the long grain (cover.hip, mtsv_coverage).
//
// The list is a fold's: n records of 6 words (read as two words, tax_id, gi, offset, edit) ordered by (read, tax_id, gi, offset).
// The table of references is sorted by key = tax_id << 32 | gi; reference r is ref_len[r] bases long and owns the words
// [word_off[r], word_off[r + 1]) of the bitmap, a whole number of words, so that no word belongs to two references.
//   k_cover_min    a lane per read: the smallest edit of its stretch [off[r], off[r + 1]) (k_pair_bounds' offsets).  A stretch of
//                  up to kCoverMinLane records is walked by its lane; a longer one is strided by the whole wavefront, one such
//                  read after the other, the minimum by shuffles.  The offsets are there anyway, and they index m by the read
//                  itself: no heads, no scan and no slots as the segmented minimum of k_lca.hip needs them.
//   k_cover_map    a lane per record: does it count, which reference is it (a binary search over the keys), does it begin a
//                  (read, tax_id, gi) run.  It writes scratch and counters only: the host refuses the call on the counters
//                  before anything is marked or added.
//   k_cover_mark   a lane per counted record.  The interval is a first-word mask, full words and a last-word mask, OR-ed into the
//                  bitmap with 64-bit atomics -- after a plain load: a word that holds the mask already is left alone, and at a
//                  hot locus that is nearly every word.  Up to lane_max words are written by the lane, a longer interval goes to
//                  a work list, a wavefront's lanes appended with one atomic.  The per-reference sums: the lanes of a wavefront
//                  that hold the reference of the first lane still waiting add up at once (k_lca_walk's leader loop), so one
//                  64-bit add a counter goes out per distinct reference and wavefront, not per lane.
//   k_cover_wave   a wavefront per entry of the work list, in a grid that strides it: the lanes stride the interval's words
//   k_cover_reads  a lane per run: a run that a counted record flagged adds one to its reference's reads, combined alike
//   k_cover_pop    a workgroup per tile of bitmap words: popcounts, the reference of a word by binary search over the word
//                  offsets, summed per reference in LDS (cell: where the reference's words begin in the tile), one global add
//                  per (tile, reference)
// Every atomic is an integer OR or add: the results do not depend on the order of arrival.
#include <hip/hip_runtime.h>

#include <string>

#include "kernels_common.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kCoverThreads = 256;
constexpr uint32_t kCoverWaves = kCoverThreads / kWave;
constexpr uint32_t kCoverNone = 0xffffffffu;
constexpr uint32_t W = 6;

// the counted record i of reference rf (< n_refs): its bases [o, end) as words w0 .. w1 of the reference; false: no base
struct CoverSpan {
    uint32_t o, w0, w1;
    uint64_t end;
};
__device__ inline bool cover_span(const uint32_t* __restrict__ rec, uint64_t i, const uint32_t* __restrict__ read_len, uint32_t L, CoverSpan* s) {
    const uint64_t read = rec_read_of<W>(rec, i);
    s->o = rec[i * W + 4];
    s->end = min((uint64_t)s->o + read_len[read], (uint64_t)L);
    if (s->end <= s->o) return false;
    s->w0 = s->o >> 6;
    s->w1 = (uint32_t)((s->end - 1) >> 6);
    return true;
}

// word w of the span into the bitmap at base + w
__device__ inline void cover_or(unsigned long long* __restrict__ bitmap, uint32_t base, const CoverSpan& s, uint32_t w) {
    const uint32_t lo = w == s.w0 ? s.o & 63 : 0, hi = w == s.w1 ? (uint32_t)((s.end - 1) & 63) : 63;
    const unsigned long long mask = (~0ull << lo) & (~0ull >> (63 - hi));
    unsigned long long* p = bitmap + ((uint64_t)base + w);
    if ((*p & mask) != mask) atomicOr(p, mask);
}

// v of the lanes in `same` summed; the same in every lane of the wavefront (all of them take part)
__device__ inline unsigned long long wave_sum_of(unsigned long long v, bool mine) {
    unsigned long long x = mine ? v : 0;
    for (int d = kWave / 2; d > 0; d >>= 1) x += (unsigned long long)__shfl_xor((long long)x, d);
    return x;
}

__global__ __launch_bounds__(kCoverThreads) void k_cover_min(const uint32_t* __restrict__ rec, uint32_t n, uint64_t n_reads, const uint32_t* __restrict__ off,
                                                            uint32_t* __restrict__ m) {
    const uint64_t r = (uint64_t)blockIdx.x * kCoverThreads + threadIdx.x;
    const bool act = r < n_reads;
    uint32_t b = 0, e = 0, x = kCoverNone;
    if (act) {
        b = min(off[r], n);
        e = min(off[r + 1], n);
    }
    const bool wide = act && e > b && e - b > kCoverMinLane;
    if (act && !wide)
        for (uint32_t j = b; j < e; j++) x = min(x, rec[(uint64_t)j * W + 5]);
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t lb = (uint32_t)__shfl((int)b, leader), le = (uint32_t)__shfl((int)e, leader);
        uint32_t y = kCoverNone;
        for (uint64_t j = (uint64_t)lb + lane_id(); j < le; j += kWave) y = min(y, rec[j * W + 5]);
        for (int d = kWave / 2; d > 0; d >>= 1) y = min(y, (uint32_t)__shfl_xor((int)y, d));
        if ((int)lane_id() == leader) x = y;
        todo &= todo - 1;
    }
    if (act) m[r] = x;
}

__global__ __launch_bounds__(kCoverThreads) void k_cover_map(const uint32_t* __restrict__ rec, uint32_t n, uint64_t n_reads, const uint32_t* __restrict__ m,
                                                            uint32_t slack, const uint64_t* __restrict__ ref_key, const uint32_t* __restrict__ ref_len,
                                                            uint32_t n_refs, uint32_t* __restrict__ ref, uint32_t* __restrict__ head,
                                                            unsigned long long* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * kCoverThreads + threadIdx.x;
    bool unknown = false, range = false, beyond = false, counted = false;
    if (i < n) {
        const uint32_t* r = rec + i * W;
        const uint64_t read = rec_read_of<W>(rec, i);
        const uint64_t key = (uint64_t)r[2] << 32 | r[3];
        beyond = read >= n_reads;
        uint32_t lo = 0, hi = n_refs;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (ref_key[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        unknown = !(lo < n_refs && ref_key[lo] == key);
        range = !unknown && r[4] >= ref_len[lo];
        if (!beyond && !unknown && !range) {
            const uint32_t best = m[read];
            const uint32_t limit = best > 0xffffffffu - slack ? 0xffffffffu : best + slack;
            counted = r[5] <= limit;
        }
        ref[i] = counted ? lo : kCoverNone;
        bool h = i == 0;
        if (!h) {
            const uint32_t* q = r - W;
            h = rec_read_of<W>(rec, i - 1) != read || q[2] != r[2] || q[3] != r[3];
        }
        head[i] = h;
    }
    const unsigned long long um = __ballot(unknown), rm = __ballot(range), ym = __ballot(beyond), cm = __ballot(counted), bad = um | rm | ym;
    if (lane_id() == 0) {
        if (um) atomicAdd(&ctr[kCoverCtrUnknown], (unsigned long long)__popcll(um));
        if (rm) atomicAdd(&ctr[kCoverCtrRange], (unsigned long long)__popcll(rm));
        if (ym) atomicAdd(&ctr[kCoverCtrBeyond], (unsigned long long)__popcll(ym));
        if (cm) atomicAdd(&ctr[kCoverCtrCounted], (unsigned long long)__popcll(cm));
        if (bad) atomicMin(&ctr[kCoverCtrFirstBad], (unsigned long long)(i + (uint32_t)__builtin_ctzll(bad)));  // (lane 0 holds i of lane 0)
    }
}

__global__ __launch_bounds__(kCoverThreads) void k_cover_mark(const uint32_t* __restrict__ rec, uint32_t n, const uint32_t* __restrict__ read_len,
                                                             const uint32_t* __restrict__ ref, const uint32_t* __restrict__ run,
                                                             const uint32_t* __restrict__ ref_len, const uint32_t* __restrict__ word_off, uint32_t n_refs,
                                                             uint32_t lane_max, unsigned long long* __restrict__ bitmap,
                                                             unsigned long long* __restrict__ cnt, uint32_t* __restrict__ run_hit,
                                                             uint32_t* __restrict__ run_ref, uint32_t* __restrict__ list,
                                                             unsigned long long* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * kCoverThreads + threadIdx.x;
    bool act = false, wide = false;
    uint32_t rf = kCoverNone;
    unsigned long long bases = 0;
    if (i < n) {
        rf = ref[i];
        act = rf < n_refs;
    }
    if (act) {
        const uint32_t s = run[i + 1] - 1;
        if (s < n) {
            run_hit[s] = 1;  // (every record of the run writes the same two values)
            run_ref[s] = rf;
        }
        CoverSpan sp;
        const uint32_t base = word_off[rf];
        if (cover_span(rec, i, read_len, ref_len[rf], &sp) && (uint64_t)base + sp.w1 < word_off[rf + 1]) {
            bases = sp.end - sp.o;
            if (sp.w1 - sp.w0 + 1 > lane_max) wide = true;
            else
                for (uint32_t w = sp.w0; w <= sp.w1; w++) cover_or(bitmap, base, sp, w);
        }
    }
    // the wavefront's records to their references, reference by reference
    unsigned long long todo = __ballot(act);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t r0 = (uint32_t)__shfl((int)rf, leader);
        const bool mine = act && rf == r0;
        const unsigned long long same = __ballot(mine);
        const unsigned long long sum = __popcll(same) > 1 ? wave_sum_of(bases, mine) : (unsigned long long)__shfl((long long)bases, leader);
        if ((int)lane_id() == leader) {
            atomicAdd(&cnt[(uint64_t)n_refs + r0], (unsigned long long)__popcll(same));
            if (sum) atomicAdd(&cnt[2 * (uint64_t)n_refs + r0], sum);
        }
        todo &= ~same;
    }
    const unsigned long long wm = __ballot(wide);
    if (wm) {
        uint32_t at0 = 0;
        if (lane_id() == 0) at0 = (uint32_t)atomicAdd(&ctr[kCoverCtrList], (unsigned long long)__popcll(wm));
        at0 = (uint32_t)__shfl((int)at0, 0);
        // (every record enters at most once: at < n whenever the caller zeroed the counter)
        const uint64_t at = (uint64_t)at0 + (uint32_t)__popcll(wm & ((1ull << lane_id()) - 1));
        if (wide && at < n) list[at] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(kCoverThreads) void k_cover_wave(const uint32_t* __restrict__ rec, uint32_t n, const uint32_t* __restrict__ read_len,
                                                             const uint32_t* __restrict__ ref, const uint32_t* __restrict__ ref_len,
                                                             const uint32_t* __restrict__ word_off, uint32_t n_refs, const uint32_t* __restrict__ list,
                                                             const unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ bitmap) {
    const uint64_t count = min((uint64_t)ctr[kCoverCtrList], (uint64_t)n);
    const uint64_t waves = (uint64_t)gridDim.x * kCoverWaves;
    for (uint64_t e = (uint64_t)blockIdx.x * kCoverWaves + threadIdx.x / kWave; e < count; e += waves) {
        const uint64_t i = list[e];
        if (i >= n) continue;
        const uint32_t rf = ref[i];
        if (rf >= n_refs) continue;
        CoverSpan sp;  // (the same in every lane)
        const uint32_t base = word_off[rf];
        if (!cover_span(rec, i, read_len, ref_len[rf], &sp) || (uint64_t)base + sp.w1 >= word_off[rf + 1]) continue;
        for (uint64_t w = (uint64_t)sp.w0 + lane_id(); w <= sp.w1; w += kWave) cover_or(bitmap, base, sp, (uint32_t)w);
    }
}

__global__ __launch_bounds__(kCoverThreads) void k_cover_reads(const unsigned long long* __restrict__ n_runs, uint32_t n, const uint32_t* __restrict__ run_hit,
                                                              const uint32_t* __restrict__ run_ref, uint32_t n_refs, unsigned long long* __restrict__ cnt) {
    const uint64_t s = (uint64_t)blockIdx.x * kCoverThreads + threadIdx.x;
    uint32_t rf = kCoverNone;
    if (s < n && s < *n_runs && run_hit[s]) rf = run_ref[s];
    const bool act = rf < n_refs;
    unsigned long long todo = __ballot(act);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t r0 = (uint32_t)__shfl((int)rf, leader);
        const unsigned long long same = __ballot(act && rf == r0);
        if ((int)lane_id() == leader) atomicAdd(&cnt[r0], (unsigned long long)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kCoverThreads) void k_cover_pop(const unsigned long long* __restrict__ bitmap, uint32_t n_words,
                                                            const uint32_t* __restrict__ word_off, uint32_t n_refs, uint32_t tile,
                                                            unsigned long long* __restrict__ cov) {
    __shared__ uint32_t s_sum[kCoverTileMax], s_ref[kCoverTileMax];  // by where a reference's words begin in the tile
    const uint64_t w_first = (uint64_t)blockIdx.x * tile;
    for (uint32_t p = threadIdx.x; p < tile; p += kCoverThreads) s_sum[p] = 0;
    __syncthreads();
    for (uint32_t p0 = 0; p0 < tile; p0 += kCoverThreads) {  // (the same trips in every lane)
        const uint64_t w = w_first + p0 + threadIdx.x;
        uint32_t c = 0, cell = 0, rf = 0;
        if (p0 + threadIdx.x < tile && w < n_words) c = (uint32_t)__popcll(bitmap[w]);
        if (c) {
            // the first reference whose words end behind w: one without a base owns no word and is never found
            uint32_t lo = 0, hi = n_refs;  // word_off[0] = 0 <= w < word_off[n_refs]
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (word_off[mid + 1] <= w) lo = mid + 1;
                else hi = mid;
            }
            rf = min(lo, n_refs - 1);
            const uint64_t begins = word_off[rf];
            cell = begins > w_first ? (uint32_t)(begins - w_first) : 0;
            if (cell >= tile) c = 0;  // (cannot be: begins <= w)
        }
        // a wavefront whose words are all of one reference -- a genome over many tiles -- sends one lane to LDS
        const unsigned long long am = __ballot(c != 0);
        if (am) {
            const int leader = __builtin_ctzll(am);
            const uint32_t cell0 = (uint32_t)__shfl((int)cell, leader);
            const unsigned long long same = __ballot(c != 0 && cell == cell0);
            if (same == am && __popcll(am) > 1) {
                uint32_t x = c;
                for (int d = kWave / 2; d > 0; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d);
                if ((int)lane_id() == leader) {
                    atomicAdd(&s_sum[cell0], x);
                    s_ref[cell0] = rf;
                }
            } else if (c) {
                atomicAdd(&s_sum[cell], c);
                s_ref[cell] = rf;  // (a cell is one reference's: every lane writes the same)
            }
        }
    }
    __syncthreads();
    for (uint32_t p = threadIdx.x; p < tile; p += kCoverThreads) {
        const uint32_t v = s_sum[p];
        if (v) atomicAdd(&cov[s_ref[p]], (unsigned long long)v);
    }
}

}  // namespace

void launch_cover_min(hipStream_t s, const void* rec, uint32_t n, uint64_t n_reads, const uint32_t* off, uint32_t* m) {
    if (!n_reads) return;
    hipLaunchKernelGGL(k_cover_min, dim3(cdiv(n_reads, kCoverThreads)), dim3(kCoverThreads), 0, s, (const uint32_t*)rec, n, n_reads, off, m);
}

void launch_cover_map(hipStream_t s, const void* rec, uint32_t n, uint64_t n_reads, const uint32_t* m, uint32_t slack, const uint64_t* ref_key,
                      const uint32_t* ref_len, uint32_t n_refs, uint32_t* ref, uint32_t* head, uint64_t* ctr) {
    if (!n) return;
    hipLaunchKernelGGL(k_cover_map, dim3(cdiv(n, kCoverThreads)), dim3(kCoverThreads), 0, s, (const uint32_t*)rec, n, n_reads, m, slack, ref_key, ref_len, n_refs,
                       ref, head, reinterpret_cast<unsigned long long*>(ctr));
}

void launch_cover_mark(hipStream_t s, const void* rec, uint32_t n, const uint32_t* read_len, const uint32_t* ref, const uint32_t* run,
                       const uint32_t* ref_len, const uint32_t* word_off, uint32_t n_refs, uint32_t lane_max, uint64_t* bitmap, uint64_t* cnt,
                       uint32_t* run_hit, uint32_t* run_ref, uint32_t* list, uint64_t* ctr) {
    if (!n || !n_refs) return;
    hipLaunchKernelGGL(k_cover_mark, dim3(cdiv(n, kCoverThreads)), dim3(kCoverThreads), 0, s, (const uint32_t*)rec, n, read_len, ref, run, ref_len, word_off,
                       n_refs, lane_max, reinterpret_cast<unsigned long long*>(bitmap), reinterpret_cast<unsigned long long*>(cnt), run_hit, run_ref, list,
                       reinterpret_cast<unsigned long long*>(ctr));
}

void launch_cover_wave(hipStream_t s, const void* rec, uint32_t n, const uint32_t* read_len, const uint32_t* ref, const uint32_t* ref_len,
                       const uint32_t* word_off, uint32_t n_refs, const uint32_t* list, const uint64_t* ctr, uint64_t* bitmap) {
    if (!n || !n_refs) return;
    // (the list's length stays on the device: a grid that strides it, at most eight workgroups per CU of a 256-CU device)
    hipLaunchKernelGGL(k_cover_wave, dim3(std::min<uint32_t>(cdiv(n, kCoverWaves), 2048)), dim3(kCoverThreads), 0, s, (const uint32_t*)rec, n, read_len, ref,
                       ref_len, word_off, n_refs, list, reinterpret_cast<const unsigned long long*>(ctr), reinterpret_cast<unsigned long long*>(bitmap));
}

void launch_cover_reads(hipStream_t s, const uint64_t* n_runs, uint32_t n, const uint32_t* run_hit, const uint32_t* run_ref, uint32_t n_refs,
                        uint64_t* cnt) {
    if (!n || !n_refs) return;
    hipLaunchKernelGGL(k_cover_reads, dim3(cdiv(n, kCoverThreads)), dim3(kCoverThreads), 0, s, reinterpret_cast<const unsigned long long*>(n_runs), n, run_hit,
                       run_ref, n_refs, reinterpret_cast<unsigned long long*>(cnt));
}

void launch_cover_pop(hipStream_t s, const uint64_t* bitmap, uint32_t n_words, const uint32_t* word_off, uint32_t n_refs, uint32_t tile, uint64_t* cov) {
    if (tile < 64 || tile > kCoverTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: coverage tile of " + std::to_string(tile) + " words");
    if (!n_words || !n_refs) return;
    hipLaunchKernelGGL(k_cover_pop, dim3(cdiv(n_words, tile)), dim3(kCoverThreads), 0, s, reinterpret_cast<const unsigned long long*>(bitmap), n_words,
                       word_off, n_refs, tile, reinterpret_cast<unsigned long long*>(cov));
}

}  // namespace mtsv
