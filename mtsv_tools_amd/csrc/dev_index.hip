// dev_index.hip -- re-pack the file's FM-index into the HBM layout (dev_layout.hpp), upload it,
// and build the two HBM-only acceleration structures the 288 GB of an MI355X make affordable:
//   * the full suffix array, reconstructed from the file's row-sampled SA by LF-walking on the
//     GPU, so that SampledSuffixArray::get (call site src/index.rs:347; ~s dependent rank queries
//     per seed hit) becomes one 4-byte gather;
//   * the SA interval of every ACGT k-mer, so that the first k of the seed_size backward-search
//     steps of FMIndex::backward_search (call site src/index.rs:305) become one 8-byte gather.
// Both hold exactly the values the reference's primitives would compute; results are unchanged.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <vector>

#include "dev_mem.hpp"
#include "kernels.hpp"

namespace mtsv {

void throw_hip(hipError_t e, const char* what, const char* file, int line) {
    throw std::runtime_error(std::string("device: ") + hipGetErrorString(e) + " at " + what + " (" + file + ":" +
                             std::to_string(line) + ")");
}

DeviceIndex::~DeviceIndex() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    (void)hipFree(d_blocks);
    (void)hipFree(d_sa_sample);
    (void)hipFree(d_sa_full);
    (void)hipFree(d_text);
    (void)hipFree(d_bin_end);
    (void)hipFree(d_bins);
    (void)hipFree(d_bin_lut);
    (void)hipFree(d_kmer);
    (void)hipFree(d_kmer_levels);
}

namespace {

inline uint32_t sym_code(uint8_t c) {
    switch (c) {
    case 'A': return kCodeA;
    case 'C': return kCodeC;
    case 'G': return kCodeG;
    case 'T': return kCodeT;
    case 'N': return kCodeN;
    case '$': return kCodeSentinel;
    default: return 7;
    }
}

// ---- acceleration-structure kernels -------------------------------------------------------

// One lane per sampled row j*s: walk LF (towards smaller text positions) writing SA values into
// every non-sampled row met, until the next sampled row or the sentinel row.  LF is one cycle over
// all rows, so every row is written exactly once.
__global__ void k_expand_sa(DevIndexView ix, uint32_t n_samples, uint32_t* __restrict__ sa_full) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_samples) return;
    uint32_t row = j * ix.sa_s;
    uint32_t v = ix.sa_sample[j];
    sa_full[row] = v;
    for (uint32_t guard = 0; guard <= ix.n; guard++) {
        uint32_t blk = row >> kBlockShift, off = row & (kBlockRows - 1);
        LoadedBlock b = load_block(ix.blocks, blk);
        uint32_t c = block_code(b, off);
        if (c == kCodeSentinel) break;  // this row is the suffix at text position 0
        row = less_of(ix, c) + block_rank(b, c, blk, off, ix.sentinel_row);
        v -= 1;
        if (row % ix.sa_s == 0) break;  // owned by another lane
        sa_full[row] = v;
    }
}

// level 1: intervals of the four single symbols
__global__ void k_kmer_level1(DevIndexView ix, uint2* __restrict__ tab) {
    uint32_t a = threadIdx.x;
    if (a >= 4) return;
    uint32_t lo = less_of(ix, a) + dev_rank(ix, a, 0);
    uint32_t hi = less_of(ix, a) + dev_rank(ix, a, ix.n);
    tab[a] = make_uint2(lo, hi);
}

// level j from level j-1: interval(aP) = LF-step(a, interval(P)); index(aP) = a*4^(j-1)+index(P)
__global__ void k_kmer_level(DevIndexView ix, const uint2* __restrict__ prev, uint2* __restrict__ cur,
                             uint32_t prev_shift) {
    // grid-stride: the last level of a 16-mer table has 2^32 entries (of a 17-mer table 2^34), more than one launch may have threads;
    // the level below has 4^(j-1) = 2^prev_shift entries
    const uint64_t total = 4ull << prev_shift, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        uint32_t a = (uint32_t)(t >> prev_shift);
        uint64_t p = t & ((1ull << prev_shift) - 1);
        uint2 iv = prev[p];
        uint32_t lo = 0, hi = 0;
        if (iv.x < iv.y) {
            uint32_t b0 = iv.x >> kBlockShift, b1 = iv.y >> kBlockShift;
            LoadedBlock B0 = load_block(ix.blocks, b0);
            lo = less_of(ix, a) + block_rank(B0, a, b0, iv.x & (kBlockRows - 1), ix.sentinel_row);
            if (b1 == b0) {
                hi = less_of(ix, a) + block_rank(B0, a, b1, iv.y & (kBlockRows - 1), ix.sentinel_row);
            } else {
                LoadedBlock B1 = load_block(ix.blocks, b1);
                hi = less_of(ix, a) + block_rank(B1, a, b1, iv.y & (kBlockRows - 1), ix.sentinel_row);
            }
        }
        cur[t] = make_uint2(lo, hi);
    }
}

// singleton entries of the finished table -> their text position and the two symbols in front of it
// (dev_layout.hpp).  The table is in k-mer order, which is SA order: lo grows with t, so the sa_full and rank-block
// reads stream; only the text byte is a random read.
__global__ void k_kmer_tag(DevIndexView ix, uint2* __restrict__ tab, uint64_t total, unsigned long long* __restrict__ n_tagged) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t mine = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint2 iv = tab[t];
        if (iv.y != iv.x + 1) continue;
        const uint32_t lo = iv.x;
        const uint32_t p = ix.sa_full[lo];
        const LoadedBlock b = load_block(ix.blocks, lo >> kBlockShift);
        const uint32_t c1 = block_code(b, lo & (kBlockRows - 1));  // text[p-1], or '$' when p == 0
        const uint32_t c2 = p >= 2 ? ix.text[p - 2] : 7u;
        tab[t] = kmer_tag_entry(p, c1, c2);
        mine++;
    }
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_tagged, (unsigned long long)mine);
}

template <class F>
void parallel_ranges(uint64_t n, int threads, F fn) {
    std::vector<std::thread> pool;
    uint64_t chunk = (n + threads - 1) / threads;
    for (int t = 0; t < threads; t++) {
        uint64_t lo = std::min(n, (uint64_t)t * chunk), hi = std::min(n, lo + chunk);
        pool.emplace_back(fn, lo, hi, t);
    }
    for (auto& th : pool) th.join();
}

}  // namespace

// The host pack: the rank blocks, the sentinel's row and the padded text codes of hx.
static void pack_on_host(const HostIndex& hx, const uint32_t n, const uint32_t n_blocks, std::vector<RankBlock>& blocks, uint64_t& sentinel_row,
                         std::vector<uint8_t>& codes) {
    int threads = (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
    if (n_blocks < 4096) threads = 1;

    // ---- pack rank blocks (two passes: per-range symbol counts, then blocks) ----------------
    blocks.resize(n_blocks);
    std::vector<std::array<uint64_t, 6>> range_cnt(threads);
    // ranges are block-aligned
    uint64_t blocks_per = ((uint64_t)n_blocks + threads - 1) / threads;
    parallel_ranges(n_blocks, threads, [&](uint64_t, uint64_t, int t) {
        uint64_t b0 = std::min<uint64_t>(n_blocks, (uint64_t)t * blocks_per), b1 = std::min<uint64_t>(n_blocks, b0 + blocks_per);
        std::array<uint64_t, 6> c{};
        uint64_t lo = b0 << kBlockShift, hi = std::min<uint64_t>(n, b1 << kBlockShift);
        for (uint64_t i = lo; i < hi; i++) {
            uint32_t code = sym_code(hx.bwt[i]);
            if (code < 6) c[code]++;
        }
        range_cnt[t] = c;
    });
    std::vector<std::array<uint64_t, 6>> range_base(threads);
    {
        std::array<uint64_t, 6> acc{};
        for (int t = 0; t < threads; t++) {
            range_base[t] = acc;
            for (int a = 0; a < 6; a++) acc[a] += range_cnt[t][a];
        }
    }
    std::vector<std::string> errs(threads);
    std::vector<uint64_t> sentinel_rows(threads, UINT64_MAX);
    static const uint8_t syms[6] = {'A', 'C', 'G', 'T', 'N', '$'};
    parallel_ranges(n_blocks, threads, [&](uint64_t, uint64_t, int t) {
        uint64_t b0 = std::min<uint64_t>(n_blocks, (uint64_t)t * blocks_per), b1 = std::min<uint64_t>(n_blocks, b0 + blocks_per);
        std::array<uint64_t, 6> c = range_base[t];
        for (uint64_t b = b0; b < b1; b++) {
            RankBlock rb;
            for (int a = 0; a < 4; a++) rb.cnt[a] = (uint32_t)c[a];
            uint64_t p0[2] = {0, 0}, p1[2] = {0, 0}, p2[2] = {0, 0};
            for (uint32_t o = 0; o < kBlockRows; o++) {
                uint64_t i = (b << kBlockShift) + o;
                uint32_t code = 7;
                if (i < n) {
                    code = sym_code(hx.bwt[i]);
                    if (code >= 6) {
                        errs[t] = "format: bwt holds a symbol outside ACGTN$";
                        return;
                    }
                    c[code]++;
                    if (code == kCodeSentinel) sentinel_rows[t] = i;
                    // cross-check the file's Occ table: checkpoint j = inclusive counts in bwt[0..=j*k]
                    if (i % hx.k == 0) {
                        uint64_t j = i / hx.k;
                        for (int a = 0; a < 6; a++)
                            if (hx.occ[syms[a]][j] != c[a]) {
                                errs[t] = "format: Occ checkpoint " + std::to_string(j) + " disagrees with the bwt";
                                return;
                            }
                    }
                }
                p0[o >> 6] |= (uint64_t)(code & 1) << (o & 63);
                p1[o >> 6] |= (uint64_t)((code >> 1) & 1) << (o & 63);
                p2[o >> 6] |= (uint64_t)((code >> 2) & 1) << (o & 63);
            }
            rb.p0[0] = p0[0]; rb.p0[1] = p0[1];
            rb.p1[0] = p1[0]; rb.p1[1] = p1[1];
            rb.p2[0] = p2[0]; rb.p2[1] = p2[1];
            blocks[b] = rb;
        }
    });
    for (auto& e : errs)
        if (!e.empty()) throw std::runtime_error(e);
    sentinel_row = UINT64_MAX;
    for (uint64_t s : sentinel_rows)
        if (s != UINT64_MAX) sentinel_row = s;
    if (sentinel_row == UINT64_MAX) throw std::runtime_error("format: bwt holds no sentinel");

    // ---- text codes ---------------------------------------------------------------------------
    codes.assign(text_padded_bytes(n), (uint8_t)7);  // padded for load16() and for the sectors of k_edit_myers (dev_layout.hpp)
    parallel_ranges(n, threads, [&](uint64_t lo, uint64_t hi, int) {
        for (uint64_t i = lo; i < hi; i++) codes[i] = (uint8_t)sym_code(hx.text[i]);
    });
}

// The device pack (k_pack.hip): d_blocks and d_text of di from the file's raw bytes, to the bytes pack_on_host makes, with its
// errors.  Uploaded raw, as temporaries: the bwt, the six Occ arrays of A C G T N $, then the text; all are freed before this
// returns (the bwt's before the text is uploaded).  The counters are read once, after the pack.  Returns the sentinel's row.
static uint64_t pack_on_device(const HostIndex& hx, const uint32_t n, const uint32_t n_blocks, DeviceIndex& di, double& copy_ms) {
    uint32_t tile = kPackTile;
    if (const char* e = getenv("MTSV_PACK_TILE")) {  // (moves the tile edges, for tests)
        const int t = atoi(e);
        if (t >= 1 && t <= (int)kPackTileMax && !(t & (t - 1))) tile = (uint32_t)t;
    }
    static const uint8_t syms[6] = {'A', 'C', 'G', 'T', 'N', '$'};
    const uint64_t n_chk = ((uint64_t)n - 1) / hx.k + 1;
    for (uint8_t a : syms)
        if (hx.occ[a].size() < n_chk) throw std::runtime_error("format: occ checkpoint count != floor((n-1)/k)+1");
    const uint32_t tiles = pack_tiles(n_blocks, tile);
    const uint64_t raw_bytes = ((uint64_t)n + 15) / 16 * 16;
    DevEvents<7> ev;  // (the temporaries are sized exactly and freed on every way out)
    DevBuf<uint8_t> d_bwt, d_raw_text;
    DevBuf<uint64_t> d_occ;
    DevBuf<uint4> d_tiles;
    DevBuf<uint32_t> d_ctr;
    ev.create();

    HIP_CHECK(hipMalloc((void**)&di.d_blocks, (uint64_t)n_blocks * sizeof(RankBlock)));
    di.bytes += (uint64_t)n_blocks * sizeof(RankBlock);
    d_bwt.alloc(raw_bytes, "the raw bwt");
    d_occ.alloc(6 * n_chk, "the raw Occ arrays");
    d_tiles.alloc(tiles, "the pack's tiles");
    d_ctr.alloc(kPackCounters, "the pack's counters");
    uint32_t ctr[kPackCounters] = {0};
    ctr[kPackCtrForeignRow] = ctr[kPackCtrOccBadFirst] = 0xffffffffu;
    double t0 = now_ms();
    HIP_CHECK(hipMemcpy(d_bwt.p, hx.bwt.data(), n, hipMemcpyHostToDevice));
    for (int a = 0; a < 6; a++)
        HIP_CHECK(hipMemcpy(d_occ.p + a * n_chk, hx.occ[syms[a]].data(), n_chk * 8, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_ctr.p, ctr, sizeof ctr, hipMemcpyHostToDevice));
    copy_ms += now_ms() - t0;

    HIP_CHECK(hipEventRecord(ev.e[0], 0));
    launch_pack_count(0, d_bwt.p, n, n_blocks, tile, d_tiles.p, d_ctr.p);
    HIP_CHECK(hipEventRecord(ev.e[1], 0));
    launch_pack_scan(0, d_tiles.p, tiles);
    HIP_CHECK(hipEventRecord(ev.e[2], 0));
    launch_pack_blocks(0, d_bwt.p, n, n_blocks, tile, d_tiles.p, di.d_blocks);
    HIP_CHECK(hipEventRecord(ev.e[3], 0));
    launch_pack_check_occ(0, di.d_blocks, n, hx.k, (uint32_t)n_chk, d_occ.p, d_ctr.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[4], 0));
    HIP_CHECK(hipMemcpy(ctr, d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost));  // (after the kernels: the null stream orders them)
    d_bwt.release();
    d_occ.release();
    d_tiles.release();
    d_ctr.release();
    // the host's order: the error of the lowest row wins, and at one row the foreign symbol comes before the checkpoint
    const uint64_t occ_row = ctr[kPackCtrOccBad] ? (uint64_t)ctr[kPackCtrOccBadFirst] * hx.k : UINT64_MAX;
    if (ctr[kPackCtrForeign] && ctr[kPackCtrForeignRow] <= occ_row) throw std::runtime_error("format: bwt holds a symbol outside ACGTN$");
    if (ctr[kPackCtrOccBad])
        throw std::runtime_error("format: Occ checkpoint " + std::to_string(ctr[kPackCtrOccBadFirst]) + " disagrees with the bwt");
    if (!ctr[kPackCtrSentinels]) throw std::runtime_error("format: bwt holds no sentinel");

    HIP_CHECK(hipMalloc((void**)&di.d_text, di.text_alloc_bytes));
    di.bytes += di.text_alloc_bytes;
    d_raw_text.alloc(raw_bytes, "the raw text");
    t0 = now_ms();
    HIP_CHECK(hipMemcpy(d_raw_text.p, hx.text.data(), n, hipMemcpyHostToDevice));
    copy_ms += now_ms() - t0;
    HIP_CHECK(hipEventRecord(ev.e[5], 0));
    launch_pack_text(0, d_raw_text.p, n, di.d_text, di.text_alloc_bytes);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ev.e[6], 0));
    HIP_CHECK(hipEventSynchronize(ev.e[6]));
    d_raw_text.release();
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // count, scan, blocks, check_occ, text
    for (int k = 0; k < 4; k++) HIP_CHECK(hipEventElapsedTime(&ms[k], ev.e[k], ev.e[k + 1]));
    HIP_CHECK(hipEventElapsedTime(&ms[4], ev.e[5], ev.e[6]));
    di.pack_ms = ms[0] + ms[1] + ms[2] + ms[3] + ms[4];
    if (getenv("MTSV_TRACE"))
        fprintf(stderr, "[upload] pack on device, tile %u: k_pack_count %.3f k_pack_scan %.3f k_pack_blocks %.3f k_pack_check_occ %.3f k_pack_text %.3f ms\n",
                tile, ms[0], ms[1], ms[2], ms[3], ms[4]);
    return ctr[kPackCtrSentinelRow];
}

std::unique_ptr<DeviceIndex> upload_index(const HostIndex& hx, int device, uint32_t flags) {
    const uint64_t n64 = hx.n();
    if (n64 >= 0xFFFFFF00ull)
        throw std::runtime_error("limit: index of 2^32 symbols or more does not fit the u32 device layout; chunk the database (mtsv-chunk)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        throw std::runtime_error("device: no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) throw std::runtime_error("device: invalid device ordinal " + std::to_string(device));
    HIP_CHECK(hipSetDevice(device));

    const uint32_t n = (uint32_t)n64;
    const uint32_t n_blocks = (n >> kBlockShift) + 1;
    // MTSV_DEV_PACK=device: uploads that do not pass the flag pack on the device too (read at every upload: an A/B switch)
    const char* pack_env = getenv("MTSV_DEV_PACK");
    const bool on_device = (flags & 4u /* MTSV_DEV_PACK_ON_DEVICE */) || (pack_env && !strcmp(pack_env, "device"));

    std::vector<RankBlock> blocks;
    std::vector<uint8_t> codes;
    uint64_t sentinel_row = UINT64_MAX;
    const double pack_t0 = now_ms();
    if (!on_device) pack_on_host(hx, n, n_blocks, blocks, sentinel_row, codes);
    const double host_pack_ms = now_ms() - pack_t0;

    // ---- SA samples, bins (on the host for both packs: n / s elements or fewer) ----------------
    std::vector<uint32_t> samp(hx.sample.size());
    for (size_t i = 0; i < samp.size(); i++) samp[i] = (uint32_t)hx.sample[i];
    std::vector<DevBin> bins(hx.bins.size());
    std::vector<uint32_t> bin_end(hx.bins.size());
    for (size_t i = 0; i < bins.size(); i++) {
        bins[i] = DevBin{(uint32_t)hx.bins[i].start, (uint32_t)hx.bins[i].end, hx.bins[i].tax_id, hx.bins[i].gi};
        bin_end[i] = (uint32_t)hx.bins[i].end;
    }

    // coarse bin lookup: bucket k covers text positions [k << shift, (k+1) << shift)
    uint32_t lut_shift = 0;
    while (((uint64_t)n >> lut_shift) > 65536) lut_shift++;
    std::vector<uint32_t> bin_lut(((uint64_t)n >> lut_shift) + 2);
    {
        uint32_t b = 0;
        for (size_t k = 0; k < bin_lut.size(); k++) {
            uint64_t p = (uint64_t)k << lut_shift;
            while (b + 1 < bins.size() && bin_end[b] <= p) b++;
            bin_lut[k] = b;
        }
    }

    auto di = std::make_unique<DeviceIndex>();
    di->device = device;
    di->flags = flags;
    double copy_ms = 0;
    auto up = [&](auto** dptr, const void* src, uint64_t bytes) {
        HIP_CHECK(hipMalloc((void**)dptr, bytes ? bytes : 16));
        const double t0 = now_ms();
        if (bytes) HIP_CHECK(hipMemcpy(*dptr, src, bytes, hipMemcpyHostToDevice));
        copy_ms += now_ms() - t0;
        di->bytes += bytes;
    };
    di->text_bytes = ((uint64_t)n + 15) / 16 * 16 + 32;  // (what MTSV_DEVPART_TEXT shows: load16()'s padding)
    di->text_alloc_bytes = text_padded_bytes(n);
    di->sa_sample_bytes = samp.size() * 4;
    di->bin_lut_bytes = bin_lut.size() * 4;
    di->packed_on_device = on_device;
    if (on_device) {
        // d_blocks and d_text from the raw bytes; every temporary is freed in there, before the k-mer table below asks
        // hipMemGetInfo what is free
        sentinel_row = pack_on_device(hx, n, n_blocks, *di, copy_ms);
        up(&di->d_sa_sample, samp.data(), samp.size() * 4);
    } else {
        di->pack_ms = (float)host_pack_ms;
        up(&di->d_blocks, blocks.data(), (uint64_t)n_blocks * sizeof(RankBlock));
        up(&di->d_sa_sample, samp.data(), samp.size() * 4);
        up(&di->d_text, codes.data(), codes.size());
    }
    up(&di->d_bin_end, bin_end.data(), bin_end.size() * 4);
    up(&di->d_bins, bins.data(), bins.size() * sizeof(DevBin));
    up(&di->d_bin_lut, bin_lut.data(), bin_lut.size() * 4);

    DevIndexView& v = di->view;
    v.blocks = di->d_blocks;
    v.n = n;
    v.n_blocks = n_blocks;
    v.C[0] = (uint32_t)hx.less['A'];
    v.C[1] = (uint32_t)hx.less['C'];
    v.C[2] = (uint32_t)hx.less['G'];
    v.C[3] = (uint32_t)hx.less['T'];
    v.C[4] = (uint32_t)hx.less['N'];
    v.sentinel_row = (uint32_t)sentinel_row;
    v.sa_sample = di->d_sa_sample;
    v.sa_s = (uint32_t)hx.s;
    v.sa_pow2_shift = 0xffffffffu;
    if (hx.s > 0xFFFFFFFFull) throw std::runtime_error("limit: suffix sampling interval does not fit u32");
    for (uint32_t sh = 0; sh < 32; sh++)
        if ((1ull << sh) == hx.s) v.sa_pow2_shift = sh;
    v.sa_full = nullptr;
    v.text = di->d_text;
    v.bin_end = di->d_bin_end;
    v.bins = di->d_bins;
    v.n_bins = (uint32_t)bins.size();
    v.bin_lut = di->d_bin_lut;
    v.bin_lut_shift = lut_shift;
    v.kmer_tab = nullptr;
    v.kmer_k = 0;

    // ---- acceleration structures ---------------------------------------------------------------
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    HIP_CHECK(hipEventRecord(e0, 0));
    if (!(flags & 1u /* MTSV_DEV_SAMPLED_SA_ONLY */)) {
        HIP_CHECK(hipMalloc((void**)&di->d_sa_full, (uint64_t)n * 4));
        di->bytes += (uint64_t)n * 4;
        uint32_t ns = (uint32_t)samp.size();
        hipLaunchKernelGGL(k_expand_sa, dim3((ns + 255) / 256), dim3(256), 0, 0, v, ns, di->d_sa_full);
        HIP_CHECK(hipGetLastError());
        v.sa_full = di->d_sa_full;
    }
    if (!(flags & 2u /* MTSV_DEV_NO_KMER_TABLE */)) {
        // table size ~ index size: 4^k entries of 8 B for 4^k <= 2n up to k = 16 (32 GiB: every symbol of the
        // table saves a dependent pair of rank-block gathers per seed), and only if it fits the free HBM twice over.
        // Indexes of 2^31 symbols or more get a 17th symbol (128 GiB) when the device has the room: that is what
        // 288 GB of HBM are for -- the 10 GB index then costs 153 GB and a default seed of 18 symbols one rank step.
        uint32_t k = 1;
        while (k < 16 && (1ull << (2 * (k + 1))) <= 2 * (uint64_t)n) k++;
        if (k == 16 && n >= (1u << 31)) k = 17;
        if (const char* e = getenv("MTSV_KMER_K")) {
            int kk = atoi(e);
            if (kk >= 1 && kk <= 17) k = (uint32_t)kk;
        }
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        // 17: the table, the level below it while building, and 48 GiB left for batch workspaces
        if (k == 17 && (10ull << 34) + (48ull << 30) > (uint64_t)free_b) k = 16;
        while (k > 1 && k <= 16 && (10ull << (2 * k)) * 2 > (uint64_t)free_b) k--;  // table + the previous level while building
        uint64_t entries = 1ull << (2 * k);
        uint2 *ta = nullptr, *tb = nullptr;
        if (k == 17) {  // 128 + 32 GiB in two pieces: free memory by the count is not always free memory in one piece
            if (hipMalloc((void**)&ta, entries * 8) != hipSuccess || hipMalloc((void**)&tb, entries / 4 * 8) != hipSuccess) {
                (void)hipGetLastError();
                if (ta) (void)hipFree(ta);
                ta = tb = nullptr;
                k = 16;
                entries = 1ull << 32;
            }
        }
        if (!ta) {
            HIP_CHECK(hipMalloc((void**)&ta, entries * 8));
            HIP_CHECK(hipMalloc((void**)&tb, std::max<uint64_t>(entries / 4, 4) * 8));
        }
        // the first levels are kept (dev_layout.hpp: kmer_level_start): a seed with an N in its table part starts from the
        // entry of the symbols behind its last N.  Each is copied as it is finished, before its buffer is written again
        // and before the table's singleton entries are tagged.
        const char* kl = getenv("MTSV_KMER_LEVELS");
        // (MTSV_KMER_LEVELS=0 builds none, for an A/B in one build; the sampled-SA mode, which is there to save memory, has none)
        const uint32_t n_levels = ((kl && atoi(kl) == 0) || !v.sa_full) ? 0 : std::min(k, kKmerLevelsMax);
        uint64_t level_bytes = 0;
        if (n_levels) {
            level_bytes = (uint64_t)kmer_level_start(n_levels + 1) * sizeof(uint2);
            HIP_CHECK(hipMalloc((void**)&di->d_kmer_levels, level_bytes));
            di->bytes += level_bytes;
        }
        auto keep_level = [&](uint32_t lvl, const uint2* src) {
            if (lvl <= n_levels)
                HIP_CHECK(hipMemcpyAsync(di->d_kmer_levels + kmer_level_start(lvl), src, (sizeof(uint2)) << (2 * lvl),
                                         hipMemcpyDeviceToDevice, 0));
        };
        // ping-pong so the last level lands in `ta`
        uint2* cur = (k % 2 == 1) ? ta : tb;
        uint2* oth = (k % 2 == 1) ? tb : ta;
        hipLaunchKernelGGL(k_kmer_level1, dim3(1), dim3(64), 0, 0, v, cur);
        keep_level(1, cur);
        for (uint32_t lvl = 2; lvl <= k; lvl++) {
            const uint64_t total = 1ull << (2 * lvl);
            hipLaunchKernelGGL(k_kmer_level, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 1u << 22)), dim3(256), 0, 0, v, cur, oth,
                               2 * (lvl - 1));
            std::swap(cur, oth);
            keep_level(lvl, cur);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipFree(tb));
        di->d_kmer = ta;  // cur == ta by construction
        di->bytes += entries * 8;
        v.kmer_tab = di->d_kmer;
        v.kmer_k = k;
        if (getenv("MTSV_TRACE"))
            fprintf(stderr, "[upload] kmer levels 1..%u kept: %llu bytes\n", n_levels, (unsigned long long)level_bytes);
        // singleton k-mers carry their text position (full SA only: the sampled-SA mode keeps its LF-walk locate)
        const char* kp = getenv("MTSV_KMER_POS");
        if (v.sa_full && !(kp && atoi(kp) == 0)) {
            unsigned long long* d_n = nullptr;
            HIP_CHECK(hipMalloc((void**)&d_n, sizeof(unsigned long long)));
            HIP_CHECK(hipMemset(d_n, 0, sizeof(unsigned long long)));
            hipEvent_t t0, t1;
            HIP_CHECK(hipEventCreate(&t0));
            HIP_CHECK(hipEventCreate(&t1));
            HIP_CHECK(hipEventRecord(t0, 0));
            hipLaunchKernelGGL(k_kmer_tag, dim3((uint32_t)std::min<uint64_t>((entries + 255) / 256, 1u << 16)), dim3(256), 0, 0, v,
                               di->d_kmer, entries, d_n);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipEventRecord(t1, 0));
            unsigned long long n_tagged = 0;
            HIP_CHECK(hipMemcpy(&n_tagged, d_n, sizeof(n_tagged), hipMemcpyDeviceToHost));
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, t0, t1));
            (void)hipEventDestroy(t0);
            (void)hipEventDestroy(t1);
            (void)hipFree(d_n);
            if (getenv("MTSV_TRACE"))
                fprintf(stderr, "[upload] kmer table k=%u: %llu tagged entries of %llu (%.1f ms)\n", k, n_tagged,
                        (unsigned long long)entries, ms);
        } else if (getenv("MTSV_TRACE")) {
            fprintf(stderr, "[upload] kmer table k=%u: 0 tagged entries of %llu (0.0 ms)\n", k, (unsigned long long)entries);
        }
    }
    HIP_CHECK(hipEventRecord(e1, 0));
    HIP_CHECK(hipEventSynchronize(e1));
    HIP_CHECK(hipEventElapsedTime(&di->accel_build_ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    di->copy_ms = (float)copy_ms;
    return di;
}

}  // namespace mtsv
