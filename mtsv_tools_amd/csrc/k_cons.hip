// k_cons.hip -- the consensus of a pileup segment (cons.hip, mtsv_pileup_consensus; the definition is in include/mtsv_amd.h,
// "consensus"), and the adds of mtsv_pileup_add_counts.  A segment is what k_pile.hip says: its references' slots one behind
// the other, [slot][8] u32 with channel 0 a difference array, tile_pre the match depth in front of every tile.
//
//   k_cons_call     a wavefront per tile of `tile` slots, 64 slots a step, shaped like k_pile_sites: channel 0 integrated with
//                   the carried prefix, then every lane classifies its slot (LOW, AMBIG, REF, SUB, DEL; INS SITE beside it) and
//                   writes one CALL BYTE: the character the position emits, 0 for a DEL and for a slot L.  tile_cnt[t] = the
//                   characters of tile t (then launch_scan: tile_off).  The lane on a reference's first slot leaves the
//                   characters of its tile in front of it in ref_pre[r].
//                   The per-reference CELLS (kConsCell u32: covered, n_ref, n_sub, n_del, n_low, n_ambig, ins_sites, a pad, and
//                   sum_depth as a u64) are zeroed by the caller.  The lanes of a step that share a reference are counted by
//                   ballots (sum_depth by a shuffle reduction) into wave-uniform registers that are kept from step to step
//                   while the reference stays; they go out with integer atomic adds when the reference changes and at the
//                   tile's end.  Integer adds only: a cell depends neither on the tile nor on the order of execution.
//   k_cons_layout   one workgroup, a lane per reference in rounds of kConsThreads: emitted or not, the header's bytes from the
//                   decimal digits of gi and TaxID, the newlines, the text's bytes; a 64-bit exclusive scan over the references,
//                   carried from round to round, gives the byte at which a reference's text begins.  lay[r] (kConsLay u32):
//                   text_off (u64), header bytes, cons_len, the characters of the segment in front of its first slot, emitted,
//                   bytes (u64).  total[0] = the bytes of the segment's text, total[1] = the emitted references.
//   k_cons_headers  a lane per emitted reference: '>' gi '-' tax_id '\n'
//   k_cons_write<STAGED>  a wavefront per tile over the call bytes: character k of its reference goes to
//                   text_off + header + k + k / line_width; the last character of a line also places the '\n'.  No byte is
//                   written twice, none outside its reference's [text_off, text_off + bytes).
//                   STAGED = false: plain byte stores.  STAGED = true: a tile that lies inside one reference owns one run of
//                   consecutive bytes of the text -- from its first character to its last, the newlines between them and the
//                   one its last character places -- and puts it together in LDS, as an image that begins on a 4-byte boundary
//                   of the text, then stores whole dwords, and single bytes in front of the first whole dword and behind the
//                   last (those dwords are shared with the neighbouring tiles).  A tile in which references meet takes the
//                   plain path.  Which of the two is the default: profiles/README.md.
//   k_cons_add      a lane per (slot, channel) of caller-given counts: channels 1 .. 7 are added as they are, channel 0 in the
//                   difference form -- slot i takes c0[i] - c0[i - 1], the slot behind the last takes -c0[last] -- so that no
//                   two lanes share an address and nothing needs an atomic.
#include <hip/hip_runtime.h>

#include <string>

#include "k_tile.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kConsThreads = 256;

// ref_off[0 .. n_refs]: the references' first slots, ascending, ref_off[n_refs] = n_slots; the reference of a slot (k_pile.hip)
__device__ inline uint32_t cons_ref_of(const uint32_t* __restrict__ ref_off, uint32_t n_refs, uint32_t slot) {
    uint32_t lo = 0, hi = n_refs;  // the last r with ref_off[r] <= slot
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ref_off[mid] <= slot) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __constant__ uint32_t kConsPow10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};
__device__ inline uint32_t cons_digits(uint32_t v) {
    uint32_t d = 1;
    while (d < 10 && v >= kConsPow10[d]) d++;
    return d;
}

struct ConsArgs {
    const uint32_t* cnt;
    uint32_t n_slots, tile;
    const uint32_t* tile_pre;
    const uint32_t* ref_off;
    uint32_t n_refs;
    const uint8_t* ref;
    uint32_t md, min_frac_ppm, fill;
    uint8_t* call;        // null: rows only
    uint32_t* tile_cnt;   // with call
    uint32_t* ref_pre;    // with call
    uint32_t* cells;
};

// the wave-uniform counters of the reference a wavefront is in
struct ConsAcc {
    uint32_t r;
    uint32_t c[7];
    unsigned long long depth;
};

__device__ inline void cons_flush(const ConsArgs& a, ConsAcc& acc) {
    if (acc.r < a.n_refs && threadIdx.x == 0) {
        uint32_t* cell = a.cells + (uint64_t)acc.r * kConsCell;
        for (int k = 0; k < 7; k++)
            if (acc.c[k]) atomicAdd(&cell[k], acc.c[k]);
        if (acc.depth) atomicAdd(reinterpret_cast<unsigned long long*>(cell + 8), acc.depth);
    }
    for (int k = 0; k < 7; k++) acc.c[k] = 0;
    acc.depth = 0;
}

__global__ __launch_bounds__(kWave) void k_cons_call(ConsArgs a) {
    const uint64_t lo = (uint64_t)blockIdx.x * a.tile, end = min(lo + a.tile, (uint64_t)a.n_slots);
    uint32_t carry = a.tile_pre[blockIdx.x], written = 0;
    const unsigned long long below = (1ull << threadIdx.x) - 1ull;
    ConsAcc acc;
    acc.r = 0xffffffffu;
    for (int k = 0; k < 7; k++) acc.c[k] = 0;
    acc.depth = 0;
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
        // the reference: one search for the step when it lies inside one reference, a search per lane otherwise
        const uint32_t rb = cons_ref_of(a.ref_off, a.n_refs, (uint32_t)base);
        uint32_t r = rb;
        if ((uint64_t)a.ref_off[rb + 1] < min(base + kWave, end) && valid) r = cons_ref_of(a.ref_off, a.n_refs, (uint32_t)s);
        const uint32_t first = a.ref_off[r], L = a.ref_off[r + 1] - first - 1, p = (uint32_t)s - first;
        const bool pos = valid && p < L;  // a position; otherwise slot L
        const uint32_t ch[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        unsigned long long depth = 0;
        for (int c = 0; c < 7; c++) depth += ch[c];
        if (!pos) depth = 0;
        uint32_t w = 0;
        for (uint32_t c = 1; c < 7; c++)
            if (ch[c] > ch[w]) w = c;
        const bool low = depth < a.md;
        const bool ambig = !low && (w == 5u || (unsigned long long)ch[w] * 1000000ull < (unsigned long long)a.min_frac_ppm * depth);
        const bool called = pos && !low && !ambig;
        const bool is_ref = called && w == 0u, is_sub = called && w >= 1u && w <= 4u, is_del = called && w == 6u;
        const bool ins = valid && ch[7] >= a.md && 2ull * ch[7] > depth;
        uint8_t out = 0;
        if (pos) {
            const uint32_t rc = min((uint32_t)a.ref[s], 4u);
            if (low || ambig) out = a.fill ? (uint8_t)"acgtn"[rc] : (uint8_t)'N';
            else if (is_ref) out = (uint8_t)"ACGTN"[rc];
            else if (is_sub) out = (uint8_t)"ACGT"[w - 1u];
        }
        if (a.call) {
            const unsigned long long m = __ballot(out != 0);
            if (valid) {
                a.call[s] = out;
                if (p == 0) a.ref_pre[r] = written + (uint32_t)__popcll(m & below);
            }
            written += (uint32_t)__popcll(m);
        }
        // the cells: the step's references one after the other (one, but where references meet)
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
            const uint32_t r0 = (uint32_t)__shfl((int)r, (int)leader);
            const bool mine = valid && r == r0;
            const unsigned long long same = __ballot(mine);
            if (r0 != acc.r) {
                cons_flush(a, acc);
                acc.r = r0;
            }
            acc.c[0] += (uint32_t)__popcll(__ballot(mine && pos && !low));  // covered
            acc.c[1] += (uint32_t)__popcll(__ballot(mine && is_ref));
            acc.c[2] += (uint32_t)__popcll(__ballot(mine && is_sub));
            acc.c[3] += (uint32_t)__popcll(__ballot(mine && is_del));
            acc.c[4] += (uint32_t)__popcll(__ballot(mine && pos && low));
            acc.c[5] += (uint32_t)__popcll(__ballot(mine && pos && ambig));
            acc.c[6] += (uint32_t)__popcll(__ballot(mine && ins));
            unsigned long long d = mine ? depth : 0ull;
            for (int k = kWave / 2; k > 0; k >>= 1) d += (unsigned long long)__shfl_xor((long long)d, k);
            acc.depth += d;
            todo &= ~same;
        }
    }
    cons_flush(a, acc);
    if (a.call && threadIdx.x == 0) a.tile_cnt[blockIdx.x] = written;
}

struct LayArgs {
    const uint32_t* cells;
    const uint32_t* ref_off;
    const uint64_t* ref_key;
    uint32_t n_refs;
    const uint32_t* ref_pre;
    const uint32_t* tile_off;  // the characters in front of every tile
    uint32_t tile;
    uint32_t min_breadth_ppm, line_width;
    uint32_t* lay;
    unsigned long long* total;
};

__global__ __launch_bounds__(kConsThreads) void k_cons_layout(LayArgs a) {
    __shared__ unsigned long long wsum[kConsThreads / kWave];
    unsigned long long carry = 0, emitted_all = 0;
    for (uint64_t r0 = 0; r0 < a.n_refs; r0 += kConsThreads) {
        const uint64_t r = r0 + threadIdx.x;
        unsigned long long bytes = 0;
        uint32_t hdr = 0, clen = 0, pre = 0;
        bool emitted = false;
        if (r < a.n_refs) {
            const uint32_t* cell = a.cells + r * kConsCell;
            const uint32_t first = a.ref_off[r], L = a.ref_off[r + 1] - first - 1, covered = cell[0];
            const uint64_t key = a.ref_key[r];
            emitted = covered >= 1u && (unsigned long long)covered * 1000000ull >= (unsigned long long)a.min_breadth_ppm * L;
            clen = L - min(cell[3], L);
            hdr = 1u + cons_digits((uint32_t)key) + 1u + cons_digits((uint32_t)(key >> 32)) + 1u;
            pre = a.tile_off[first / a.tile] + a.ref_pre[r];
            const unsigned long long lines = a.line_width ? ((unsigned long long)clen + a.line_width - 1) / a.line_width : (clen ? 1ull : 0ull);
            if (emitted) bytes = (unsigned long long)hdr + clen + lines;
        }
        // the workgroup's exclusive sum of bytes
        unsigned long long incl = bytes;
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned long long up = (unsigned long long)__shfl_up((long long)incl, d);
            if ((int)lane_id() >= d) incl += up;
        }
        __syncthreads();  // (the last round's wsum has been read)
        if (lane_id() == (uint32_t)kWave - 1) wsum[threadIdx.x / kWave] = incl;
        __syncthreads();
        unsigned long long before = incl - bytes, all = 0;
        for (uint32_t w = 0; w < kConsThreads / kWave; w++) {
            if (w < threadIdx.x / kWave) before += wsum[w];
            all += wsum[w];
        }
        if (r < a.n_refs) {
            const unsigned long long at = carry + before;
            uint32_t* q = a.lay + r * kConsLay;
            q[0] = (uint32_t)at;
            q[1] = (uint32_t)(at >> 32);
            q[2] = hdr;
            q[3] = clen;
            q[4] = pre;
            q[5] = emitted ? 1u : 0u;
            q[6] = (uint32_t)bytes;
            q[7] = (uint32_t)(bytes >> 32);
        }
        carry += all;
        emitted_all += (unsigned long long)__popcll(__ballot(emitted));
    }
    // (emitted_all holds this wavefront's count)
    __syncthreads();
    if (lane_id() == 0) wsum[threadIdx.x / kWave] = emitted_all;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long n = 0;
        for (uint32_t w = 0; w < kConsThreads / kWave; w++) n += wsum[w];
        a.total[0] = carry;
        a.total[1] = n;
    }
}

__device__ inline uint64_t cons_put_decimal(uint8_t* __restrict__ text, uint64_t at, uint32_t v) {
    const uint32_t n = cons_digits(v);
    for (uint32_t k = 0; k < n; k++) {
        text[at + n - 1 - k] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
    return at + n;
}

__global__ __launch_bounds__(kConsThreads) void k_cons_headers(const uint32_t* __restrict__ lay, const uint64_t* __restrict__ ref_key, uint32_t n_refs,
                                                               uint8_t* __restrict__ text, uint64_t text_bytes) {
    const uint64_t r = (uint64_t)blockIdx.x * kConsThreads + threadIdx.x;
    if (r >= n_refs) return;
    const uint32_t* q = lay + r * kConsLay;
    if (!q[5]) return;
    uint64_t at = (uint64_t)q[0] | (uint64_t)q[1] << 32;
    if (at + q[2] > text_bytes) return;  // (cannot be: the layout counted these bytes)
    const uint64_t key = ref_key[r];
    text[at++] = (uint8_t)'>';
    at = cons_put_decimal(text, at, (uint32_t)key);
    text[at++] = (uint8_t)'-';
    at = cons_put_decimal(text, at, (uint32_t)(key >> 32));
    text[at] = (uint8_t)'\n';
}

struct WriteArgs {
    const uint8_t* call;
    uint32_t n_slots, tile;
    const uint32_t* tile_off;
    const uint32_t* ref_off;
    uint32_t n_refs;
    const uint32_t* lay;
    uint32_t line_width;
    uint8_t* text;
    uint64_t text_bytes;
};

constexpr uint32_t kConsStage = 2 * kPileTileMax + 8;  // bytes: a tile's characters, a newline each at most, and the alignment

template <bool STAGED>
__global__ __launch_bounds__(kWave) void k_cons_write(WriteArgs a) {
    __shared__ uint32_t stage[STAGED ? kConsStage / 4 : 1];
    const uint64_t lo = (uint64_t)blockIdx.x * a.tile, end = min(lo + a.tile, (uint64_t)a.n_slots);
    uint32_t written = a.tile_off[blockIdx.x];
    const unsigned long long below = (1ull << threadIdx.x) - 1ull;
    if (STAGED) {
        const uint32_t r = cons_ref_of(a.ref_off, a.n_refs, (uint32_t)lo);
        const uint32_t n_chars = a.tile_off[blockIdx.x + 1] - written;
        if ((uint64_t)a.ref_off[r + 1] >= end) {  // the tile lies inside reference r (the whole wavefront decides alike)
            const uint32_t* q = a.lay + (uint64_t)r * kConsLay;
            if (!q[5] || !n_chars) return;
            const uint32_t clen = q[3], k0 = written - q[4], k1 = k0 + n_chars - 1;  // the tile's first and last character
            const uint64_t body = ((uint64_t)q[0] | (uint64_t)q[1] << 32) + q[2];
            const uint64_t g0 = body + k0 + (a.line_width ? k0 / a.line_width : 0u);
            const bool last_ends = k1 + 1u == clen || (a.line_width && (k1 + 1u) % a.line_width == 0u);
            const uint64_t g1 = body + k1 + (a.line_width ? k1 / a.line_width : 0u) + 1u + (last_ends ? 1u : 0u);
            const uint64_t a0 = g0 & ~3ull;
            if (k0 <= k1 && k1 < clen && g1 <= a.text_bytes && g1 - a0 <= kConsStage) {  // (cannot fail: the layout counted these bytes)
                uint8_t* const img = reinterpret_cast<uint8_t*>(stage);
                uint32_t run = 0;
                for (uint64_t base = lo; base < end; base += kWave) {
                    const uint64_t s = base + threadIdx.x;
                    const uint8_t c = s < end ? a.call[s] : (uint8_t)0;
                    const unsigned long long m = __ballot(c != 0);
                    if (c) {
                        const uint32_t k = k0 + run + (uint32_t)__popcll(m & below);
                        const uint64_t at = body + k + (a.line_width ? k / a.line_width : 0u);
                        if (k <= k1) {
                            img[at - a0] = c;
                            if (k + 1u == clen || (a.line_width && (k + 1u) % a.line_width == 0u)) img[at + 1 - a0] = (uint8_t)'\n';
                        }
                    }
                    run += (uint32_t)__popcll(m);
                }
                __syncthreads();
                const uint64_t d0 = min((g0 + 3) & ~3ull, g1), d1 = max(g1 & ~3ull, d0);  // whole dwords of the run: [d0, d1)
                for (uint64_t b = g0 + threadIdx.x; b < d0; b += kWave) a.text[b] = img[b - a0];
                uint32_t* const out = reinterpret_cast<uint32_t*>(a.text);
                for (uint64_t w = (d0 >> 2) + threadIdx.x; w < (d1 >> 2); w += kWave) out[w] = stage[w - (a0 >> 2)];
                for (uint64_t b = d1 + threadIdx.x; b < g1; b += kWave) a.text[b] = img[b - a0];
                return;
            }
        }
    }
    for (uint64_t base = lo; base < end; base += kWave) {
        const uint64_t s = base + threadIdx.x;
        const uint8_t c = s < end ? a.call[s] : (uint8_t)0;
        const unsigned long long m = __ballot(c != 0);
        if (c) {
            const uint32_t r = cons_ref_of(a.ref_off, a.n_refs, (uint32_t)s);
            const uint32_t* q = a.lay + (uint64_t)r * kConsLay;
            if (q[5]) {
                const uint32_t k = written + (uint32_t)__popcll(m & below) - q[4], clen = q[3];
                const uint64_t at = ((uint64_t)q[0] | (uint64_t)q[1] << 32) + q[2] + k + (a.line_width ? k / a.line_width : 0u);
                const bool line_end = k + 1u == clen || (a.line_width && (k + 1u) % a.line_width == 0u);
                if (k < clen && at + (line_end ? 1u : 0u) < a.text_bytes) {  // (cannot fail: the layout counted these bytes)
                    a.text[at] = c;
                    if (line_end) a.text[at + 1] = (uint8_t)'\n';
                }
            }
        }
        written += (uint32_t)__popcll(m);
    }
}

// counts: [n][8] as a download gives them; cnt: the reference's first slot's counters; first + n <= slots
__global__ __launch_bounds__(kConsThreads) void k_cons_add(uint32_t* __restrict__ cnt, uint32_t slots, uint32_t first, uint64_t n,
                                                           const uint32_t* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * kConsThreads + threadIdx.x;
    const uint64_t k = i >> 3;
    const uint32_t c = (uint32_t)i & 7u;
    if (k > n) return;
    const uint64_t slot = (uint64_t)first + k;
    if (slot >= slots) return;  // (the slot behind slot L: its difference is zero, the caller checked slot L's channel 0)
    if (c) {
        if (k < n) cnt[slot * 8 + c] += counts[k * 8 + c];
    } else {
        const uint32_t here = k < n ? counts[k * 8] : 0u, prev = k ? counts[(k - 1) * 8] : 0u;
        cnt[slot * 8] += here - prev;
    }
}

void check_cons_tile(uint32_t tile) {
    if (tile < 64 || tile > kPileTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: a pileup tile of " + std::to_string(tile) + " slots");
}

}  // namespace

void launch_cons_call(hipStream_t s, const uint32_t* cnt, uint32_t n_slots, uint32_t tile, const uint32_t* tile_pre, const uint32_t* ref_off, uint32_t n_refs,
                      const uint8_t* ref, uint32_t md, uint32_t min_frac_ppm, uint32_t fill, uint8_t* call, uint32_t* tile_cnt, uint32_t* ref_pre,
                      uint32_t* cells) {
    check_cons_tile(tile);
    if (!n_slots || !n_refs) return;
    const ConsArgs a{cnt, n_slots, tile, tile_pre, ref_off, n_refs, ref, md, min_frac_ppm, fill, call, tile_cnt, ref_pre, cells};
    hipLaunchKernelGGL(k_cons_call, dim3(pile_tiles(n_slots, tile)), dim3(kWave), 0, s, a);
}

void launch_cons_layout(hipStream_t s, const uint32_t* cells, const uint32_t* ref_off, const uint64_t* ref_key, uint32_t n_refs, const uint32_t* ref_pre,
                        const uint32_t* tile_off, uint32_t tile, uint32_t min_breadth_ppm, uint32_t line_width, uint32_t* lay, uint64_t* total) {
    check_cons_tile(tile);
    const LayArgs a{cells, ref_off, ref_key, n_refs, ref_pre, tile_off, tile, min_breadth_ppm, line_width, lay, reinterpret_cast<unsigned long long*>(total)};
    hipLaunchKernelGGL(k_cons_layout, dim3(1), dim3(kConsThreads), 0, s, a);
}

void launch_cons_write(hipStream_t s, const uint8_t* call, uint32_t n_slots, uint32_t tile, const uint32_t* tile_off, const uint32_t* ref_off,
                       const uint64_t* ref_key, uint32_t n_refs, const uint32_t* lay, uint32_t line_width, uint8_t* text, uint64_t text_bytes, bool staged) {
    check_cons_tile(tile);
    if (!n_slots || !n_refs || !text_bytes) return;
    hipLaunchKernelGGL(k_cons_headers, dim3(cdiv(n_refs, kConsThreads)), dim3(kConsThreads), 0, s, lay, ref_key, n_refs, text, text_bytes);
    const WriteArgs a{call, n_slots, tile, tile_off, ref_off, n_refs, lay, line_width, text, text_bytes};
    if (staged) hipLaunchKernelGGL(k_cons_write<true>, dim3(pile_tiles(n_slots, tile)), dim3(kWave), 0, s, a);
    else hipLaunchKernelGGL(k_cons_write<false>, dim3(pile_tiles(n_slots, tile)), dim3(kWave), 0, s, a);
}

void launch_cons_add(hipStream_t s, uint32_t* cnt, uint32_t slots, uint32_t first, uint64_t n, const uint32_t* counts) {
    if (!n) return;
    hipLaunchKernelGGL(k_cons_add, dim3(cdiv((n + 1) * 8, kConsThreads)), dim3(kConsThreads), 0, s, cnt, slots, first, n, counts);
}

}  // namespace mtsv
