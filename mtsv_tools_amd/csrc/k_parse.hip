// k_parse.hip -- the inverse of k_text.hip: the hit parts of result lines, which lie in HBM as text, become a sorted list of
// assignment records with distinct keys, as k_collapse leaves a run (parse.hip, mtsv_fold_add_text).
//
// The text is `hits`, N bytes: the hit parts of n_lines lines end to end, line j = hits[line_off[j] .. line_off[j + 1]),
// TOKEN(,TOKEN)* or nothing, read number line_read[j].  A token is T=E, T-G=E or T-G-O=E, every number 1 to 10 decimal
// digits with value <= 2^32 - 1: at most 43 bytes.  line_off ascends from 0 (the host has checked that).
//
// Byte-parallel, then record-parallel; no lane walks a line or a run of equal keys:
//   k_parse<false>  a workgroup owns `tile` bytes (a power of two, 64 .. kParseTileMax).  The tile goes to LDS with 16-byte
//                   loads.  A byte STARTS A TOKEN when it begins a non-empty line or the byte before it is ',' -- for the
//                   tile's first byte that is the byte before it in global memory, so two neighbouring tiles decide an edge
//                   from the same bytes.  tile_cnt[t] = the starts of tile t        (then launch_scan: tile_off, the tokens)
//   k_parse<true>   the same, 48 more bytes behind the tile (never past N), then a scan of the start flags; every start's
//                   lane parses its token from LDS -- at most 44 bytes, whatever they hold -- and writes a raw token at
//                   tile_off[t] + rank: key (read, tax, gi, offset) and val (edit, first of its line, line).  Outside the
//                   grammar -- and, when the grain needs GI and offset, without them; a ',' that ends its line -- is counted,
//                   the smallest such line kept by atomicMin.
//                   THE LINE OF A TOKEN: two lanes find the lines of the tile's first and last byte by binary search in
//                   line_off; a token searches between them.  The other way -- marking line starts in LDS and ranking them --
//                   needs a second scan and a rule for empty lines (any number of them share one offset); the search needs
//                   neither: the last line whose offset is not above the byte is the non-empty one, and the range is a
//                   handful of lines unless the lines are a few bytes each.
//   k_parse_heads   a lane per raw token: flag[i] = it is the first of its line or its key at the grain differs from its
//                   predecessor's.  Counted apart, with the smallest line, for the host to refuse: a key below its
//                   predecessor's inside a line; a line whose read is not above the previous non-empty line's; a read at or
//                   above n_reads                                                   (then launch_scan over the flags: place)
//   k_parse_place   a head writes its record at place[i]: the key fields, and all ones where the value goes; its TaxID apart
//   k_parse_reduce  every token does one 64-bit atomicMin of its value into the record of its run, out[place[i] + flag[i] - 1].
//                   The value is the record's last 8 bytes as they lie: offset below edit in the wide grains -- the smaller
//                   (edit, offset) for TAXID_GI; LONG's runs share the offset -- and tax_id below edit in the narrow one.  The
//                   heads' stores are complete before the first atomic: the two are launches of one stream.  So a line of
//                   thousands of tokens of one key costs what thousands of lines do, and no tile edge needs a rule.
#include <hip/hip_runtime.h>

#include <string>

#include "k_tile.hpp"

namespace mtsv {
namespace {

constexpr uint32_t kParseThreads = 256;
constexpr uint32_t kParseOver = 48;   // bytes behind the tile in LDS: a token that starts in the tile ends inside them
constexpr uint32_t kParseWalk = 44;   // bytes a lane looks at: a canonical token and what ends it
constexpr uint32_t kParseMisc = 64;   // bytes in front of the tile in LDS: [0], [1] u64 the lines of the tile's first and last byte; u32 [8 ..] the wavefronts' sums
constexpr uint32_t kParsePre = 16;    // the byte before the tile lies at buf[kParsePre - 1]

// the last line whose offset is not above g, searched among lines [lo, hi] (line lo's offset is not above g)
__device__ inline uint64_t parse_line_of(const uint64_t* __restrict__ line_off, uint64_t lo, uint64_t hi, uint64_t g) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1) >> 1);
        if (line_off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct ParseTok {
    uint32_t tax, gi, off, edit, fields;
    bool bad;
};

// the token at b (LDS), of which `lim` bytes may be looked at (the rest of its line, or kParseWalk); *len: its bytes
// without what ends it, *comma: a ',' ends it
__device__ inline ParseTok parse_token(const uint8_t* b, uint32_t lim, uint32_t* len, bool* comma) {
    ParseTok t{0, 0, 0, 0, 0, false};
    uint32_t f = 0, nd = 0, k = 0;
    uint64_t v = 0;
    bool eq = false;
    *comma = false;
    for (; k < lim; k++) {
        const uint32_t c = b[k];
        if (c == ',') {
            *comma = true;
            break;
        }
        if (c - '0' < 10u) {
            nd++;
            if (nd <= 10) v = v * 10 + (c - '0');
            if (nd > 10 || v > 0xffffffffull) t.bad = true;
        } else if (c == '-' || c == '=') {
            if (eq || nd == 0 || (c == '-' && f >= 2)) t.bad = true;
            if (f == 0) t.tax = (uint32_t)v;
            else if (f == 1) t.gi = (uint32_t)v;
            else t.off = (uint32_t)v;
            if (c == '=') eq = true;
            else f++;
            nd = 0;
            v = 0;
        } else {
            t.bad = true;
        }
    }
    if (!eq || nd == 0) t.bad = true;
    if (!*comma && k == kParseWalk) t.bad = true;  // (nothing ends it where a canonical token has ended)
    t.edit = (uint32_t)v;
    t.fields = f + 1;
    *len = k;
    return t;
}

template <bool WRITE>
__global__ __launch_bounds__(kParseThreads) void k_parse(const uint8_t* __restrict__ hits, uint64_t N, const uint64_t* __restrict__ line_off,
                                                        const uint32_t* __restrict__ line_read, uint64_t n_lines, uint32_t tile, int wide,
                                                        uint32_t* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_off, uint32_t n_tok,
                                                        uint4* __restrict__ raw_key, uint4* __restrict__ raw_val,
                                                        unsigned long long* __restrict__ ctr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t parse_lds[];
    uint64_t* edge = reinterpret_cast<uint64_t*>(parse_lds);
    uint32_t* wsum = reinterpret_cast<uint32_t*>(parse_lds) + 8;
    uint8_t* buf = parse_lds + kParseMisc;                      // buf[kParsePre + p] = byte g0 + p
    uint8_t* mark = buf + kParsePre + tile + kParseOver;        // mark[p]: byte g0 + p begins a non-empty line
    const uint64_t g0 = (uint64_t)blockIdx.x * tile;
    const uint32_t nt = (uint32_t)min((uint64_t)tile, N - g0);
    const uint64_t g1 = g0 + nt;
    // ---- the lines of the tile's first and last byte; the tile and what follows it to LDS ----
    if (threadIdx.x < 2) edge[threadIdx.x] = parse_line_of(line_off, 0, n_lines - 1, threadIdx.x ? g1 - 1 : g0);
    const uint64_t gl = WRITE ? min(g1 + kParseOver, N) : g1;  // bytes [g0, gl) are loaded
    const uint32_t nl = (uint32_t)(gl - g0);
    for (uint32_t q = threadIdx.x; q * 16 < nl; q += kParseThreads) {
        if (q * 16 + 16 <= nl) {
            *reinterpret_cast<uint4*>(buf + kParsePre + q * 16) = *reinterpret_cast<const uint4*>(hits + g0 + q * 16);
        } else {
            for (uint32_t k = q * 16; k < nl; k++) buf[kParsePre + k] = hits[g0 + k];
        }
    }
    if (threadIdx.x == 0) buf[kParsePre - 1] = g0 ? hits[g0 - 1] : (uint8_t)0;
    for (uint32_t p = threadIdx.x; p < nt; p += kParseThreads) mark[p] = 0;
    __syncthreads();
    const uint64_t j_lo = edge[0], j_hi = edge[1];
    // (the lines between the two, consecutive lanes consecutive lines: a non-empty one begins at a byte of its own)
    for (uint64_t j = j_lo + threadIdx.x; j <= j_hi; j += kParseThreads) {
        const uint64_t o = line_off[j];
        if (o >= g0 && o < g1 && line_off[j + 1] > o) mark[o - g0] = 1;
    }
    __syncthreads();

    // ---- the token starts: a stretch of bytes per lane, the lanes' counts summed by block_excl_sum ----
    const uint32_t ipt = max(tile / kParseThreads, 1u);
    const uint32_t p0 = min(threadIdx.x * ipt, nt), p1 = min(p0 + ipt, nt);
    uint32_t mine = 0;
    for (uint32_t p = p0; p < p1; p++) mine += mark[p] | (buf[kParsePre - 1 + p] == ',');
    const BlockSum sum = block_excl_sum<kParseThreads>(mine, wsum);
    if (!WRITE) {
        if (threadIdx.x == 0) tile_cnt[blockIdx.x] = sum.total;
        return;
    }
    uint32_t before = sum.before;

    // ---- every start's token: parsed from LDS, written at tile_off + rank ----
    const uint64_t base = tile_off[blockIdx.x], end = min((uint64_t)tile_off[blockIdx.x + 1], (uint64_t)n_tok);
    uint32_t n_bad = 0;
    uint64_t bad_line = ~0ull;
    for (uint32_t p = p0; p < p1; p++) {
        if (!(mark[p] | (buf[kParsePre - 1 + p] == ','))) continue;
        const uint64_t o = base + before++;
        const uint64_t g = g0 + p;
        const uint64_t line = parse_line_of(line_off, j_lo, j_hi, g);
        const uint64_t line_end = line_off[line + 1];
        const uint32_t lim = (uint32_t)min(line_end - g, (uint64_t)kParseWalk);
        uint32_t len;
        bool comma;
        ParseTok t = parse_token(buf + kParsePre + p, lim, &len, &comma);
        if (comma && g + len + 1 == line_end) t.bad = true;  // (a ',' with no token behind it)
        if (wide && t.fields != 3) t.bad = true;
        if (t.bad) {
            n_bad++;
            bad_line = min(bad_line, line);
        }
        if (o >= end) continue;  // (a tile writes inside the stretch the count pass gave it)
        raw_key[o] = make_uint4(line_read[line], t.tax, t.gi, t.off);
        raw_val[o] = make_uint4(t.edit, mark[p], (uint32_t)line, (uint32_t)(line >> 32));
    }
    if (n_bad) {
        atomicAdd(&ctr[kParseCtrFormat], (unsigned long long)n_bad);
        atomicMin(&ctr[kParseCtrFormat + 1], (unsigned long long)bad_line);
    }
}

// the key of a raw token at the grain below its predecessor's (-1), equal (0) or above (1)
template <int G>
__device__ inline int parse_key_cmp(const uint4& k, const uint4& p) {
    if (k.y != p.y) return k.y < p.y ? -1 : 1;
    if (G == kCollapseGrainTaxid) return 0;
    if (k.z != p.z) return k.z < p.z ? -1 : 1;
    if (G == kCollapseGrainTaxidGi) return 0;
    if (k.w != p.w) return k.w < p.w ? -1 : 1;
    return 0;
}

template <int G>
__global__ __launch_bounds__(kParseThreads) void k_parse_heads(const uint4* __restrict__ raw_key, const uint4* __restrict__ raw_val, uint32_t n_tok,
                                                              uint64_t n_reads, uint32_t* __restrict__ flag,
                                                              unsigned long long* __restrict__ ctr) {
    const uint64_t i = (uint64_t)blockIdx.x * kParseThreads + threadIdx.x;
    if (i >= n_tok) return;
    const uint4 k = raw_key[i], v = raw_val[i];
    const unsigned long long line = (unsigned long long)v.z | (unsigned long long)v.w << 32;
    const bool first = v.y != 0;
    bool head = true;
    if (i) {
        const uint4 p = raw_key[i - 1];
        if (first) {
            if (k.x <= p.x) {
                atomicAdd(&ctr[kParseCtrReadOrder], 1ull);
                atomicMin(&ctr[kParseCtrReadOrder + 1], line);
            }
        } else {
            const int c = parse_key_cmp<G>(k, p);
            head = c != 0;
            if (c < 0) {
                atomicAdd(&ctr[kParseCtrKeyOrder], 1ull);
                atomicMin(&ctr[kParseCtrKeyOrder + 1], line);
            }
        }
    }
    if (first && k.x >= n_reads) {
        atomicAdd(&ctr[kParseCtrReadRange], 1ull);
        atomicMin(&ctr[kParseCtrReadRange + 1], line);
    }
    flag[i] = head;
}

template <int G>
__global__ __launch_bounds__(kParseThreads) void k_parse_place(const uint4* __restrict__ raw_key, const uint32_t* __restrict__ flag,
                                                              const uint32_t* __restrict__ place, uint32_t n_tok, uint32_t n_rec,
                                                              uint32_t* __restrict__ out, uint32_t* __restrict__ tax_out) {
    const uint64_t i = (uint64_t)blockIdx.x * kParseThreads + threadIdx.x;
    if (i >= n_tok || !flag[i]) return;
    const uint64_t o = place[i];
    if (o >= n_rec) return;
    const uint4 k = raw_key[i];
    tax_out[o] = k.y;
    if (G == kCollapseGrainTaxid) {
        *reinterpret_cast<uint4*>(out + o * 4) = make_uint4(k.x, 0u, k.y, 0xffffffffu);
        return;
    }
    uint32_t* dst = out + o * 6;
    if (!(o & 1)) {  // (24-byte records: every other one begins on a 16-byte boundary)
        *reinterpret_cast<uint4*>(dst) = make_uint4(k.x, 0u, k.y, k.z);
        *reinterpret_cast<uint2*>(dst + 4) = make_uint2(0xffffffffu, 0xffffffffu);
    } else {
        *reinterpret_cast<uint2*>(dst) = make_uint2(k.x, 0u);
        *reinterpret_cast<uint4*>(dst + 2) = make_uint4(k.y, k.z, 0xffffffffu, 0xffffffffu);
    }
}

template <int G>
__global__ __launch_bounds__(kParseThreads) void k_parse_reduce(const uint4* __restrict__ raw_key, const uint4* __restrict__ raw_val,
                                                               const uint32_t* __restrict__ flag, const uint32_t* __restrict__ place, uint32_t n_tok,
                                                               uint32_t n_rec, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kParseThreads + threadIdx.x;
    if (i >= n_tok) return;
    const uint64_t o = (uint64_t)place[i] + flag[i] - 1;  // (token 0 is a head: place 0, flag 1)
    if (o >= n_rec) return;
    const uint4 k = raw_key[i];
    const unsigned long long edit = raw_val[i].x;
    // (8-byte aligned: 16 * o + 8, 24 * o + 16)
    if (G == kCollapseGrainTaxid) atomicMin(reinterpret_cast<unsigned long long*>(out + o * 4 + 2), edit << 32 | k.y);
    else atomicMin(reinterpret_cast<unsigned long long*>(out + o * 6 + 4), edit << 32 | k.w);
}

void parse_check(int grain) {
    if (grain != kCollapseGrainTaxid && grain != kCollapseGrainTaxidGi && grain != kCollapseGrainLong)
        throw std::runtime_error("internal: parse at grain " + std::to_string(grain));
}

}  // namespace

uint32_t parse_tiles(uint64_t n_bytes, uint32_t tile) { return cdiv(n_bytes, tile); }

void launch_parse_count(hipStream_t s, const uint8_t* hits, uint64_t n_bytes, const uint64_t* line_off, uint64_t n_lines, uint32_t tile,
                        uint32_t* tile_cnt) {
    if (tile < 64 || tile > kParseTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: parse tile of " + std::to_string(tile) + " bytes");
    const uint32_t tiles = parse_tiles(n_bytes, tile);
    if (!tiles || !n_lines) return;
    const uint32_t lds = kParseMisc + kParsePre + 2 * tile + kParseOver;
    hipLaunchKernelGGL(k_parse<false>, dim3(tiles), dim3(kParseThreads), lds, s, hits, n_bytes, line_off, (const uint32_t*)nullptr, n_lines, tile, 0,
                       tile_cnt, (const uint32_t*)nullptr, 0u, (uint4*)nullptr, (uint4*)nullptr, (unsigned long long*)nullptr);
}

void launch_parse_tokens(hipStream_t s, int grain, const uint8_t* hits, uint64_t n_bytes, const uint64_t* line_off, const uint32_t* line_read,
                         uint64_t n_lines, uint32_t tile, const uint32_t* tile_off, uint32_t n_tok, void* raw_key, void* raw_val, uint64_t* ctr) {
    parse_check(grain);
    if (tile < 64 || tile > kParseTileMax || (tile & (tile - 1))) throw std::runtime_error("internal: parse tile of " + std::to_string(tile) + " bytes");
    const uint32_t tiles = parse_tiles(n_bytes, tile);
    if (!tiles || !n_lines || !n_tok) return;
    const uint32_t lds = kParseMisc + kParsePre + 2 * tile + kParseOver;
    hipLaunchKernelGGL(k_parse<true>, dim3(tiles), dim3(kParseThreads), lds, s, hits, n_bytes, line_off, line_read, n_lines, tile,
                       grain != kCollapseGrainTaxid ? 1 : 0, (uint32_t*)nullptr, tile_off, n_tok, (uint4*)raw_key, (uint4*)raw_val,
                       reinterpret_cast<unsigned long long*>(ctr));
}

void launch_parse_heads(hipStream_t s, int grain, const void* raw_key, const void* raw_val, uint32_t n_tok, uint64_t n_reads, uint32_t* flag,
                        uint64_t* ctr) {
    parse_check(grain);
    if (!n_tok) return;
    const dim3 grid(cdiv(n_tok, kParseThreads)), block(kParseThreads);
    auto* c = reinterpret_cast<unsigned long long*>(ctr);
    const uint4 *k = (const uint4*)raw_key, *v = (const uint4*)raw_val;
    if (grain == kCollapseGrainTaxid) hipLaunchKernelGGL(k_parse_heads<kCollapseGrainTaxid>, grid, block, 0, s, k, v, n_tok, n_reads, flag, c);
    else if (grain == kCollapseGrainLong) hipLaunchKernelGGL(k_parse_heads<kCollapseGrainLong>, grid, block, 0, s, k, v, n_tok, n_reads, flag, c);
    else hipLaunchKernelGGL(k_parse_heads<kCollapseGrainTaxidGi>, grid, block, 0, s, k, v, n_tok, n_reads, flag, c);
}

void launch_parse_reduce(hipStream_t s, int grain, const void* raw_key, const void* raw_val, const uint32_t* flag, const uint32_t* place,
                         uint32_t n_tok, uint32_t n_rec, void* out, uint32_t* tax_out) {
    parse_check(grain);
    if (!n_tok || !n_rec) return;
    const dim3 grid(cdiv(n_tok, kParseThreads)), block(kParseThreads);
    const uint4 *k = (const uint4*)raw_key, *v = (const uint4*)raw_val;
    uint32_t* o = (uint32_t*)out;
    if (grain == kCollapseGrainTaxid) {
        hipLaunchKernelGGL(k_parse_place<kCollapseGrainTaxid>, grid, block, 0, s, k, flag, place, n_tok, n_rec, o, tax_out);
        hipLaunchKernelGGL(k_parse_reduce<kCollapseGrainTaxid>, grid, block, 0, s, k, v, flag, place, n_tok, n_rec, o);
    } else if (grain == kCollapseGrainLong) {
        hipLaunchKernelGGL(k_parse_place<kCollapseGrainLong>, grid, block, 0, s, k, flag, place, n_tok, n_rec, o, tax_out);
        hipLaunchKernelGGL(k_parse_reduce<kCollapseGrainLong>, grid, block, 0, s, k, v, flag, place, n_tok, n_rec, o);
    } else {
        hipLaunchKernelGGL(k_parse_place<kCollapseGrainTaxidGi>, grid, block, 0, s, k, flag, place, n_tok, n_rec, o, tax_out);
        hipLaunchKernelGGL(k_parse_reduce<kCollapseGrainTaxidGi>, grid, block, 0, s, k, v, flag, place, n_tok, n_rec, o);
    }
}

}  // namespace mtsv
