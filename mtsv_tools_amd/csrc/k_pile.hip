// k_pile.hip -- the pileup of placed hits: per reference position what the reads that align over it show there (pile.hip,
// mtsv_pileup; the definition is in include/mtsv_amd.h, "pileup").
//
// A reference of L bases owns L + 1 SLOTS of eight u32 counters, slot-major: [slot][0 .. 8) = match, A, C, G, T, N, del, ins.
// Slot L takes insertions behind the last base only.  The references of a SEGMENT lie one behind the other.
//
// Channel 0 is kept as a DIFFERENCE array: a run of n '=' from position j adds +1 at slot j and -1 (+0xffffffff, the arithmetic
// is u32 and wraps) at slot j + n, which is at most L and so inside the same reference.  The match depth of a position is the
// prefix sum of channel 0 up to it; every run closes inside its reference, so the prefix sum is zero again behind every
// reference's slot L and one plain scan over a whole segment needs no segmentation.  A clean read costs two atomics.
//
//   k_pile_best   a lane per hit: atomicMin of its edit into best[its resident read] (best preset to all ones)
//   k_pile_count  a lane per hit: skipped (its bin has no counters: the TaxID list does not select it) or counted
//                 (edit <= best + slack, saturating); two counters, nothing else is written
//   k_pile        a lane per counted hit walks its ops (k_place's, in reference order) and its read's codes on the hit's
//                 strand: '=' run two atomics, X / D one per base, I one per run.  Every index is checked against the
//                 reference's slots before the add; a script that would leave them (none: k_place keeps ref_end within the
//                 bin) stops and is counted in [kPileCtrBroken].
//                 Equal addresses inside a wavefront are NOT combined before the atomic: see profiles/README.md.
//   k_pile_ref    a lane per slot of a new segment: the text's code (0 .. 4), 0xff for a slot L
//   k_pile_tile_sums   a wavefront per tile of `tile` slots: the wrapped sum of channel 0        (then launch_scan: tile_pre)
//   k_pile_sites<M>    a wavefront per tile, 64 slots a step: channel 0 integrated with the carried prefix, then
//                      M = count: the site predicate, tile_cnt[t] = the tile's sites              (then launch_scan: tile_off)
//                      M = rows:  the same again, row tile_off[t] + rank for every site
//                      M = dump:  [slot][8] with channel 0 integrated, for the slots of one reference
// Every atomic is an integer add or min on a u32: the counters are exact and depend neither on the order of execution nor on
// the tile.  Every store is a plain vector store.
#include <hip/hip_runtime.h>

#include <string>

#include "k_tile.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kPileThreads = 256;

__device__ inline uint32_t pile_limit(uint32_t best, uint32_t slack) {
    const uint32_t s = best + slack;
    return s < best ? 0xffffffffu : s;
}

__global__ __launch_bounds__(kPileThreads) void k_pile_best(const DevHit* __restrict__ hits, uint32_t n, const uint32_t* __restrict__ hit_read,
                                                            uint32_t n_reads, uint32_t* __restrict__ best) {
    const uint64_t i = (uint64_t)blockIdx.x * kPileThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = hit_read[i];
    if (r < n_reads) atomicMin(&best[r], hits[i].edit);
}

__global__ __launch_bounds__(kPileThreads) void k_pile_count(const DevHit* __restrict__ hits, uint32_t n, const uint32_t* __restrict__ hit_bin,
                                                             const uint32_t* __restrict__ hit_read, uint32_t n_bins, uint32_t n_reads,
                                                             const uint32_t* __restrict__ best, uint32_t slack, uint32_t* const* __restrict__ bin_cnt,
                                                             unsigned long long* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * kPileThreads + threadIdx.x;
    bool skipped = false, counted = false;
    if (i < n) {
        const uint32_t b = hit_bin[i], r = hit_read[i];
        if (b < n_bins && r < n_reads) {
            skipped = bin_cnt[b] == nullptr;
            counted = !skipped && hits[i].edit <= pile_limit(best[r], slack);
        }
    }
    const unsigned long long cm = __ballot(counted), sm = __ballot(skipped);
    if (lane_id() == 0) {
        if (cm) atomicAdd(&ctr[kPileCtrCounted], (unsigned long long)__popcll(cm));
        if (sm) atomicAdd(&ctr[kPileCtrSkipped], (unsigned long long)__popcll(sm));
    }
}

struct PileArgs {
    const DevHit* hits;
    uint32_t n;
    const uint32_t* hit_bin;
    const uint32_t* hit_read;
    const DevBin* bins;
    uint32_t n_bins, n_reads;
    const uint32_t* best;
    uint32_t slack;
    uint32_t* const* bin_cnt;  // per bin of the workspace's index: its reference's counters, or null
    const uint8_t* codes;
    const uint32_t* read_off;
    const uint32_t* out;  // 12 words per hit: mtsv_placement
    const uint32_t* ops;
    uint64_t n_ops_total;
    unsigned long long* ctr;
};

__global__ __launch_bounds__(kPileThreads) void k_pile(PileArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kPileThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t bi = a.hit_bin[i], r = a.hit_read[i];
    if (bi >= a.n_bins || r >= a.n_reads) return;  // (cannot be: the placement refused such a hit)
    uint32_t* const c = a.bin_cnt[bi];
    if (!c) return;
    const DevHit h = a.hits[i];
    if (h.edit > pile_limit(a.best[r], a.slack)) return;
    const DevBin bin = a.bins[bi];
    const uint32_t Lref = bin.end - bin.start;  // slots 0 .. Lref
    const uint32_t ro = a.read_off[r], L = a.read_off[r + 1] - ro;
    const uint8_t* const rd = a.codes + ro;
    const uint32_t* const o = a.out + i * 12;
    const uint32_t n_ops = o[8];
    const uint64_t ops_off = (uint64_t)o[10] | (uint64_t)o[11] << 32;
    uint32_t ri = 0;
    uint64_t j = o[6];  // ref_start
    bool broken = ops_off + n_ops > a.n_ops_total;
    for (uint32_t k = 0; k < n_ops && !broken; k++) {
        const uint32_t op = a.ops[ops_off + k], len = op >> 4, code = op & 15u;
        if (code == 7u) {  // '=': +1 at the run's first position, -1 behind its last
            if (j + len > Lref || ri + len > L) {
                broken = true;
            } else {
                atomicAdd(&c[j * 8], 1u);
                atomicAdd(&c[(j + len) * 8], 0xffffffffu);
                ri += len;
                j += len;
            }
        } else if (code == 8u) {  // 'X': the read's base on the hit's strand
            if (j + len > Lref || ri + len > L) {
                broken = true;
            } else {
                for (uint32_t t = 0; t < len; t++, ri++, j++) atomicAdd(&c[j * 8 + 1 + min(strand_code(rd, L, h.strand, ri), 4u)], 1u);
            }
        } else if (code == 2u) {  // 'D'
            if (j + len > Lref) {
                broken = true;
            } else {
                for (uint32_t t = 0; t < len; t++, j++) atomicAdd(&c[j * 8 + 6], 1u);
            }
        } else if (code == 1u) {  // 'I': once per run, at the slot of the reference base behind it
            if (j > Lref || ri + len > L) {
                broken = true;
            } else {
                atomicAdd(&c[j * 8 + 7], 1u);
                ri += len;
            }
        } else {
            broken = true;
        }
    }
    if (broken) atomicAdd(&a.ctr[kPileCtrBroken], 1ull);
}

// ref_off[0 .. n_refs]: the references' first slots, ascending, ref_off[n_refs] = n_slots; the reference of a slot
__device__ inline uint32_t pile_ref_of(const uint32_t* __restrict__ ref_off, uint32_t n_refs, uint32_t slot) {
    uint32_t lo = 0, hi = n_refs;  // the last r with ref_off[r] <= slot
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ref_off[mid] <= slot) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kPileThreads) void k_pile_ref(const uint8_t* __restrict__ text, const uint32_t* __restrict__ ref_off,
                                                           const uint32_t* __restrict__ text_start, uint32_t n_refs, uint32_t n_slots,
                                                           uint8_t* __restrict__ ref) {
    const uint64_t s = (uint64_t)blockIdx.x * kPileThreads + threadIdx.x;
    if (s >= n_slots || !n_refs) return;
    const uint32_t r = pile_ref_of(ref_off, n_refs, (uint32_t)s);
    const uint32_t p = (uint32_t)s - ref_off[r], len = ref_off[r + 1] - ref_off[r] - 1;
    ref[s] = p < len ? (uint8_t)min((uint32_t)text[(uint64_t)text_start[r] + p], 4u) : (uint8_t)0xff;
}

__global__ __launch_bounds__(kWave) void k_pile_tile_sums(const uint32_t* __restrict__ cnt, uint32_t n_slots, uint32_t tile,
                                                          uint32_t* __restrict__ tile_sum) {
    const uint64_t lo = (uint64_t)blockIdx.x * tile, end = min(lo + tile, (uint64_t)n_slots);
    uint32_t s = 0;
    for (uint64_t at = lo + threadIdx.x; at < end; at += kWave) s += cnt[at * 8];
    for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s;
}

struct SitesArgs {
    const uint32_t* cnt;
    uint32_t n_slots, tile;
    const uint32_t* tile_pre;  // the match depth in front of each tile
    uint32_t min_depth, min_alt, min_alt_ppm;
    uint32_t* tile_cnt;        // count
    const uint32_t* tile_off;  // rows
    const uint32_t* ref_off;
    const uint64_t* ref_key;
    uint32_t n_refs;
    const uint8_t* ref;
    uint32_t* rows;  // 12 words per row: mtsv_pile_site
    uint64_t n_rows;
    uint32_t* dump;  // dump: [slot - dump_lo][8]
    uint32_t dump_lo, dump_hi;
};

constexpr int kSitesCount = 0, kSitesRows = 1, kSitesDump = 2;

template <int M>
__global__ __launch_bounds__(kWave) void k_pile_sites(SitesArgs a) {
    const uint64_t lo = (uint64_t)blockIdx.x * a.tile, end = min(lo + a.tile, (uint64_t)a.n_slots);
    if (M == kSitesDump && (end <= a.dump_lo || lo >= a.dump_hi)) return;  // (the whole wavefront)
    uint32_t carry = a.tile_pre[blockIdx.x], written = 0;
    const unsigned long long below = (1ull << threadIdx.x) - 1ull;
    for (uint64_t base = lo; base < end; base += kWave) {
        const uint64_t s = base + threadIdx.x;
        const bool valid = s < end;
        uint4 x = make_uint4(0, 0, 0, 0), y = x;
        if (valid) {
            const uint4* p = reinterpret_cast<const uint4*>(a.cnt + s * 8);
            x = p[0];
            y = p[1];
        }
        const uint32_t incl = wave_incl_sum(x.x);
        x.x = carry + incl;
        carry += __shfl(incl, kWave - 1);
        if (M == kSitesDump) {
            if (valid && s >= a.dump_lo && s < a.dump_hi) {
                uint4* q = reinterpret_cast<uint4*>(a.dump + (s - a.dump_lo) * 8);
                q[0] = x;
                q[1] = y;
            }
            continue;
        }
        const uint32_t ch[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        uint64_t depth = 0;
        for (int c = 0; c < 7; c++) depth += ch[c];
        bool alt = false;
        for (int c = 1; c < 8; c++) alt |= ch[c] >= a.min_alt && (uint64_t)ch[c] * 1000000ull >= (uint64_t)a.min_alt_ppm * depth;
        const bool site = valid && depth + ch[7] > 0 && depth >= a.min_depth && alt;
        const unsigned long long m = __ballot(site);
        if (M == kSitesRows && site) {
            const uint64_t row = (uint64_t)a.tile_off[blockIdx.x] + written + (uint32_t)__popcll(m & below);
            if (row < a.n_rows) {  // (cannot fail: the count pass saw the same counters)
                const uint32_t r = pile_ref_of(a.ref_off, a.n_refs, (uint32_t)s);
                const uint64_t key = a.ref_key[r];
                uint4* q = reinterpret_cast<uint4*>(a.rows + row * 12);
                q[0] = make_uint4((uint32_t)(key >> 32), (uint32_t)key, (uint32_t)s - a.ref_off[r], (uint32_t)a.ref[s]);
                q[1] = x;
                q[2] = y;
            }
        }
        written += (uint32_t)__popcll(m);
    }
    if (M == kSitesCount && threadIdx.x == 0) a.tile_cnt[blockIdx.x] = written;
}

}  // namespace

void launch_pile_best(hipStream_t s, const DevHit* hits, uint32_t n, const uint32_t* hit_read, uint32_t n_reads, uint32_t* best) {
    if (!n) return;
    hipLaunchKernelGGL(k_pile_best, dim3(cdiv(n, kPileThreads)), dim3(kPileThreads), 0, s, hits, n, hit_read, n_reads, best);
}

void launch_pile_count(hipStream_t s, const DevHit* hits, uint32_t n, const uint32_t* hit_bin, const uint32_t* hit_read, uint32_t n_bins, uint32_t n_reads,
                       const uint32_t* best, uint32_t slack, uint32_t* const* bin_cnt, uint64_t* ctr) {
    if (!n) return;
    hipLaunchKernelGGL(k_pile_count, dim3(cdiv(n, kPileThreads)), dim3(kPileThreads), 0, s, hits, n, hit_bin, hit_read, n_bins, n_reads, best, slack, bin_cnt,
                       reinterpret_cast<unsigned long long*>(ctr));
}

void launch_pile(hipStream_t s, const DevHit* hits, uint32_t n, const uint32_t* hit_bin, const uint32_t* hit_read, const DevBin* bins, uint32_t n_bins,
                 uint32_t n_reads, const uint32_t* best, uint32_t slack, uint32_t* const* bin_cnt, const uint8_t* codes, const uint32_t* read_off,
                 const void* out, const uint32_t* ops, uint64_t n_ops_total, uint64_t* ctr) {
    if (!n) return;
    const PileArgs a{hits, n, hit_bin, hit_read, bins, n_bins, n_reads, best, slack, bin_cnt, codes, read_off, (const uint32_t*)out, ops, n_ops_total,
                     reinterpret_cast<unsigned long long*>(ctr)};
    hipLaunchKernelGGL(k_pile, dim3(cdiv(n, kPileThreads)), dim3(kPileThreads), 0, s, a);
}

void launch_pile_ref(hipStream_t s, const uint8_t* text, const uint32_t* ref_off, const uint32_t* text_start, uint32_t n_refs, uint32_t n_slots, uint8_t* ref) {
    if (!n_slots || !n_refs) return;
    hipLaunchKernelGGL(k_pile_ref, dim3(cdiv(n_slots, kPileThreads)), dim3(kPileThreads), 0, s, text, ref_off, text_start, n_refs, n_slots, ref);
}

uint32_t pile_tiles(uint32_t n_slots, uint32_t tile) { return cdiv(n_slots, tile); }

static void check_pile_tile(uint32_t tile) {
    if (tile < 64 || tile > kPileTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: a pileup tile of " + std::to_string(tile) + " slots");
}

void launch_pile_tile_sums(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, uint32_t* tile_sum) {
    check_pile_tile(tile);
    if (!n_slots) return;
    hipLaunchKernelGGL(k_pile_tile_sums, dim3(pile_tiles(n_slots, tile)), dim3(kWave), 0, s, cnt, n_slots, tile, tile_sum);
}

void launch_pile_sites_count(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, const uint32_t* tile_pre, uint32_t min_depth, uint32_t min_alt,
                             uint32_t min_alt_ppm, uint32_t* tile_cnt) {
    check_pile_tile(tile);
    if (!n_slots) return;
    SitesArgs a{};
    a.cnt = cnt, a.n_slots = n_slots, a.tile = tile, a.tile_pre = tile_pre, a.min_depth = min_depth, a.min_alt = min_alt, a.min_alt_ppm = min_alt_ppm;
    a.tile_cnt = tile_cnt;
    hipLaunchKernelGGL(k_pile_sites<kSitesCount>, dim3(pile_tiles(n_slots, tile)), dim3(kWave), 0, s, a);
}

void launch_pile_sites_rows(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, const uint32_t* tile_pre, uint32_t min_depth, uint32_t min_alt,
                            uint32_t min_alt_ppm, const uint32_t* tile_off, const uint32_t* ref_off, const uint64_t* ref_key, uint32_t n_refs, const uint8_t* ref,
                            void* rows, uint64_t n_rows) {
    check_pile_tile(tile);
    if (!n_slots || !n_rows || !n_refs) return;
    SitesArgs a{};
    a.cnt = cnt, a.n_slots = n_slots, a.tile = tile, a.tile_pre = tile_pre, a.min_depth = min_depth, a.min_alt = min_alt, a.min_alt_ppm = min_alt_ppm;
    a.tile_off = tile_off, a.ref_off = ref_off, a.ref_key = ref_key, a.n_refs = n_refs, a.ref = ref, a.rows = (uint32_t*)rows, a.n_rows = n_rows;
    hipLaunchKernelGGL(k_pile_sites<kSitesRows>, dim3(pile_tiles(n_slots, tile)), dim3(kWave), 0, s, a);
}

void launch_pile_dump(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, const uint32_t* tile_pre, uint32_t lo, uint32_t hi, uint32_t* dump) {
    check_pile_tile(tile);
    if (!n_slots || lo >= hi || hi > n_slots) return;
    SitesArgs a{};
    a.cnt = cnt, a.n_slots = n_slots, a.tile = tile, a.tile_pre = tile_pre, a.dump = dump, a.dump_lo = lo, a.dump_hi = hi;
    hipLaunchKernelGGL(k_pile_sites<kSitesDump>, dim3(pile_tiles(n_slots, tile)), dim3(kWave), 0, s, a);
}

}  // namespace mtsv
