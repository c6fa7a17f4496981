// capi.cpp -- the extern "C" boundary declared in include/mtsv_amd.h.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mtsv_amd.h"
#include "abund_rows.hpp"
#include "batch.hpp"
#include "cons_rows.hpp"
#include "cover.hpp"
#include "dedup.hpp"
#include "dev_index.hpp"
#include "fold.hpp"
#include "mgindex.hpp"
#include "pile.hpp"

using namespace mtsv;

static thread_local std::string g_err;
static int g_build_device = -1;  // mtsv_set_build_device

static int fail(const std::exception& e) {
    g_err = e.what();
    auto starts = [&](const char* p) { return g_err.rfind(p, 0) == 0; };
    if (starts("io:")) return MTSV_E_IO;
    if (starts("format:")) return MTSV_E_FORMAT;
    if (starts("device:")) return MTSV_E_DEVICE;
    if (starts("limit:")) return MTSV_E_LIMIT;
    if (starts("nomem:")) return MTSV_E_NOMEM;
    if (starts("arg:")) return MTSV_E_ARG;
    return MTSV_E_DEVICE;
}
static int fail_arg(const char* msg) {
    g_err = std::string("arg: ") + msg;
    return MTSV_E_ARG;
}
#define GUARD(...)                           \
    try {                                    \
        __VA_ARGS__;                         \
        return MTSV_OK;                      \
    } catch (const std::bad_alloc&) {        \
        g_err = "nomem: host allocation";    \
        return MTSV_E_NOMEM;                 \
    } catch (const std::exception& e) {      \
        return fail(e);                      \
    }

// a vector as an array for mtsv_free
template <class T>
static T* malloc_copy(const std::vector<T>& v) {
    T* mem = (T*)malloc(std::max<size_t>(v.size(), 1) * sizeof(T));
    if (!mem) throw std::bad_alloc();
    if (!v.empty()) memcpy(mem, v.data(), v.size() * sizeof(T));
    return mem;
}

namespace {
struct SplitMix64 {
    uint64_t s;
    explicit SplitMix64(uint64_t seed) : s(seed) {}
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t n) { return n ? (uint64_t)(((unsigned __int128)next() * n) >> 64) : 0; }
    bool chance(double p) { return (next() >> 11) * (1.0 / 9007199254740992.0) < p; }
};
inline uint64_t mix(uint64_t a, uint64_t b) { return SplitMix64(a ^ (b * 0xD6E8FEB86659FD93ull + 0x2545F4914F6CDD1Dull)).next(); }

template <class F>
void par_for(uint64_t n, int threads, F fn) {
    if (threads < 1) threads = 1;
    std::vector<std::thread> pool;
    uint64_t chunk = (n + threads - 1) / threads;
    for (int t = 0; t < threads; t++) {
        uint64_t lo = std::min(n, (uint64_t)t * chunk), hi = std::min(n, lo + chunk);
        if (lo < hi) pool.emplace_back(fn, lo, hi);
    }
    for (auto& th : pool) th.join();
}
}  // namespace

namespace {
// run fn(k) for k in [0, n) on one thread each; the first failure (by k) is rethrown in the caller
template <class F>
void fork_join(int n, F fn) {
    std::vector<std::string> err(n);
    std::vector<char> bad(n, 0);
    std::vector<std::thread> th;
    auto body = [&](int k) {
        try {
            fn(k);
        } catch (const std::exception& e) {
            err[k] = e.what();
            bad[k] = 1;
        }
    };
    for (int k = 1; k < n; k++) th.emplace_back(body, k);
    body(0);
    for (auto& t : th) t.join();
    for (int k = 0; k < n; k++)
        if (bad[k]) throw std::runtime_error(err[k]);
}
// slot of entry k: how many earlier entries name the same device
int slot_of(const int* devices, int k) {
    int s = 0;
    for (int j = 0; j < k; j++) s += devices[j] == devices[k];
    return s;
}
void release_parts(std::vector<mtsv_hit*>& parts) {
    for (auto*& p : parts) {
        if (p && !mtsv::pinned_hits_release(p)) free(p);
        p = nullptr;
    }
}
}  // namespace

extern "C" {

const char* mtsv_last_error(void) { return g_err.c_str(); }
const char* mtsv_version(void) { return "mtsv_tools_amd 0.1.0 (gfx950)"; }

void mtsv_params_default(mtsv_params* p) {  // src/bin/mtsv-binner.rs:63-94
    p->edit_rate = 0.13;
    p->seed_size = 18;
    p->seed_interval = 15;
    p->min_seed = 0.015;
    p->max_hits = 2000;
    p->tune_max_hits = 200;
    p->max_assignments = -1;
    p->max_candidates = -1;
}

int mtsv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mtsv_index_load(const char* path, mtsv_index** out) {
    if (!path || !out) return fail_arg("null argument");
    GUARD({
        auto ix = std::make_unique<mtsv_index>();
        load_index(path, ix->host);
        *out = ix.release();
    })
}

int mtsv_index_build(uint64_t n_seqs, const uint32_t* tax_ids, const uint32_t* gis, const uint8_t* const* seqs,
                     const uint64_t* seq_lens, uint32_t occ_k, uint64_t sa_s, int n_threads, mtsv_index** out) {
    if (!out || (n_seqs && (!tax_ids || !gis || !seqs || !seq_lens))) return fail_arg("null argument");
    GUARD({
        std::vector<SeqEntry> e(n_seqs);
        for (uint64_t i = 0; i < n_seqs; i++) e[i] = SeqEntry{tax_ids[i], gis[i], seqs[i], seq_lens[i]};
        auto ix = std::make_unique<mtsv_index>();
        build_index(std::move(e), occ_k, sa_s, n_threads, ix->host, g_build_device);
        *out = ix.release();
    })
}

int mtsv_set_build_device(int hip_device) {
    g_build_device = hip_device;
    return MTSV_OK;
}

int mtsv_index_build_fasta(const char* fasta_path, uint32_t occ_k, uint64_t sa_s, int n_threads, mtsv_index** out) {
    if (!fasta_path || !out) return fail_arg("null argument");
    GUARD({
        auto ix = std::make_unique<mtsv_index>();
        build_index_from_fasta(fasta_path, occ_k, sa_s, n_threads, ix->host, g_build_device);
        *out = ix.release();
    })
}

int mtsv_index_write(const mtsv_index* ix, const char* path) {
    if (!ix || !path) return fail_arg("null argument");
    GUARD({
        write_index(ix->host, path);
        const_cast<mtsv_index*>(ix)->host.file_bytes = 0;
    })
}

int mtsv_index_info(const mtsv_index* ix, mtsv_index_info_t* info) {
    if (!ix || !info) return fail_arg("null argument");
    info->n = ix->host.n();
    info->n_bins = ix->host.bins.size();
    info->occ_k = ix->host.k;
    info->sa_s = ix->host.s;
    info->file_bytes = ix->host.file_bytes;
    info->device_bytes = 0;
    info->kmer_k = 0;
    info->sa_full = 0;
    for (auto& kv : ix->dev) {
        info->device_bytes = kv.second->bytes;
        info->kmer_k = kv.second->view.kmer_tab ? kv.second->view.kmer_k : 0;
        info->sa_full = kv.second->view.sa_full ? 1 : 0;
    }
    return MTSV_OK;
}

void mtsv_index_free(mtsv_index* ix) {
    if (!ix) return;
    for (auto& kv : ix->cached_batch) delete kv.second->b;
    delete ix;
}

int mtsv_index_to_device(mtsv_index* ix, int hip_device, uint32_t flags) {
    if (!ix) return fail_arg("null index");
    GUARD({
        std::lock_guard<std::mutex> lk(ix->mu);
        auto it = ix->dev.find(hip_device);
        if (it == ix->dev.end() || it->second->flags != flags) {
            for (auto cb = ix->cached_batch.begin(); cb != ix->cached_batch.end();) {
                if (cb->first.first == hip_device) {
                    {
                        std::lock_guard<std::mutex> wl(cb->second->mu);  // no call may be running on it
                        delete cb->second->b;
                        cb->second->b = nullptr;
                    }
                    cb = ix->cached_batch.erase(cb);
                } else
                    ++cb;
            }
            if (it != ix->dev.end()) ix->dev.erase(it);
            ix->dev[hip_device] = upload_index(ix->host, hip_device, flags);
        }
    })
}

static DeviceIndex* device_index(mtsv_index* ix, int dev) {
    auto it = ix->dev.find(dev);
    if (it == ix->dev.end()) throw std::runtime_error("arg: index is not resident on device " + std::to_string(dev) + " (call mtsv_index_to_device)");
    return it->second.get();
}

int mtsv_index_download_device(mtsv_index* ix, int hip_device, int part, void** out, uint64_t* bytes) {
    if (!ix || !out || !bytes) return fail_arg("null argument");
    GUARD({
        std::lock_guard<std::mutex> lk(ix->mu);
        const DeviceIndex* di = device_index(ix, hip_device);
        const DevIndexView& v = di->view;
        mtsv_device_header h;
        memset(&h, 0, sizeof h);
        const void* src = nullptr;
        uint64_t len = 0;
        switch (part) {
        case MTSV_DEVPART_HEADER:
            h.n = v.n;
            h.n_blocks = v.n_blocks;
            for (int a = 0; a < 5; a++) h.C[a] = v.C[a];
            h.sentinel_row = v.sentinel_row;
            h.sa_s = v.sa_s;
            h.sa_pow2_shift = v.sa_pow2_shift;
            h.n_bins = v.n_bins;
            h.bin_lut_shift = v.bin_lut_shift;
            h.kmer_k = v.kmer_tab ? v.kmer_k : 0;
            h.sa_full = v.sa_full ? 1 : 0;
            h.packed_on_device = di->packed_on_device ? 1 : 0;
            h.device_bytes = di->bytes;
            h.pack_ms = di->pack_ms;
            h.copy_ms = di->copy_ms;
            h.accel_build_ms = di->accel_build_ms;
            len = sizeof h;
            break;
        case MTSV_DEVPART_BLOCKS: src = di->d_blocks, len = (uint64_t)v.n_blocks * sizeof(RankBlock); break;
        case MTSV_DEVPART_TEXT: src = di->d_text, len = di->text_bytes; break;
        case MTSV_DEVPART_TEXT_SECTORS: src = di->d_text, len = di->text_alloc_bytes; break;
        case MTSV_DEVPART_SA_SAMPLE: src = di->d_sa_sample, len = di->sa_sample_bytes; break;
        case MTSV_DEVPART_BINS: src = di->d_bins, len = (uint64_t)v.n_bins * sizeof(DevBin); break;
        case MTSV_DEVPART_BIN_END: src = di->d_bin_end, len = (uint64_t)v.n_bins * 4; break;
        case MTSV_DEVPART_BIN_LUT: src = di->d_bin_lut, len = di->bin_lut_bytes; break;
        default: throw std::runtime_error("arg: unknown MTSV_DEVPART_* " + std::to_string(part));
        }
        void* p = malloc(len ? len : 1);
        if (!p) throw std::bad_alloc();
        if (part == MTSV_DEVPART_HEADER) {
            memcpy(p, &h, sizeof h);
        } else if (len) {
            hipError_t e = hipSetDevice(hip_device);
            if (e == hipSuccess) e = hipMemcpy(p, src, len, hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                free(p);
                throw std::runtime_error(std::string("device: ") + hipGetErrorString(e) + " at mtsv_index_download_device");
            }
        }
        *out = p;
        *bytes = len;
    })
}

int mtsv_batch_create(mtsv_index* ix, int hip_device, uint64_t max_reads, uint64_t max_bases, uint64_t max_hits_ws,
                      mtsv_batch** out) {
    if (!ix || !out) return fail_arg("null argument");
    GUARD({
        std::lock_guard<std::mutex> lk(ix->mu);
        *out = new mtsv_batch(ix, device_index(ix, hip_device), max_reads, max_bases, max_hits_ws);
    })
}

int mtsv_batch_create_lanes(mtsv_index* ix, int hip_device, uint64_t max_reads, uint64_t max_bases, uint64_t max_hits_ws, int lanes,
                            mtsv_batch** out) {
    if (!ix || !out || lanes < 0) return fail_arg("null argument");
    GUARD({
        std::lock_guard<std::mutex> lk(ix->mu);
        *out = new mtsv_batch(ix, device_index(ix, hip_device), max_reads, max_bases, max_hits_ws, nullptr, lanes);
    })
}

int mtsv_batch_reserve_host(mtsv_batch* b, uint64_t n_reads, uint64_t n_bases, uint32_t warm_read_len) {
    if (!b) return fail_arg("null argument");
    GUARD({
        b->impl.reserve_host(n_reads, n_bases);
        // (the warm-up reads are not the caller's: they stay out of a taxa report that is already on)
        struct ReportOff {
            bool& on;
            const bool was;
            explicit ReportOff(bool& o) : on(o), was(o) { on = false; }
            ~ReportOff() { on = was; }
        } report_off(b->impl.report.on);
        // (nor are they a run whose match flags anybody asked for; and they go through the gather kernels whatever the mode)
        struct MatchOff {
            int& mode;
            const int was;
            explicit MatchOff(int& m) : mode(m), was(m) { mode = MTSV_MATCH_OFF; }
            ~MatchOff() { mode = was; }
        } match_off(b->impl.match.mode);
        const std::vector<uint8_t>& text = b->impl.ix->host.text;
        if (warm_read_len && text.size() >= (uint64_t)warm_read_len * 2 + 16) {
            // reads sampled from the index through every kernel once: the first launch of a kernel loads its code object,
            // the first pass of a lane sizes its seed arrays
            const uint64_t n = std::min<uint64_t>(std::max<uint64_t>(n_reads, 1), std::max<uint64_t>(4096, (uint64_t)b->impl.n_lanes * 32768));
            std::vector<uint8_t> bases(n * warm_read_len);
            std::vector<uint64_t> off(n + 1);
            if (mtsv_synth_reads(b->impl.ix, 0x7761726d, n, warm_read_len, bases.data(), off.data()) != MTSV_OK)
                throw std::runtime_error(std::string("internal: ") + mtsv_last_error());
            mtsv_params p;
            mtsv_params_default(&p);
            b->impl.run_host(bases.data(), off.data(), n, p);
            mtsv_hit* h = nullptr;
            uint64_t nh = 0;
            b->impl.download(&h, &nh);
            mtsv_hits_free(h);
        }
    })
}

int mtsv_batch_upload(mtsv_batch* b, const uint8_t* bases, const uint64_t* read_off, uint64_t n_reads) {
    if (!b || !read_off || (!bases && n_reads && read_off[n_reads] != read_off[0])) return fail_arg("null argument");
    GUARD(b->impl.upload(bases, read_off, n_reads))
}

int mtsv_batch_run(mtsv_batch* b, const mtsv_params* params) {
    if (!b || !params) return fail_arg("null argument");
    GUARD(b->impl.run(*params))
}

int mtsv_batch_run_host(mtsv_batch* b, const uint8_t* bases, const uint64_t* read_off, uint64_t n_reads,
                        const mtsv_params* params) {
    if (!b || !read_off || !params || (!bases && n_reads && read_off[n_reads] > read_off[0])) return fail_arg("null argument");
    GUARD(b->impl.run_host(bases, read_off, n_reads, *params))
}

int mtsv_batch_run_host_parts(mtsv_batch* b, int n_parts, const uint8_t* const* bases, const uint64_t* const* read_off,
                              const uint64_t* n_reads, const mtsv_params* params) {
    if (!b || n_parts < 0 || (n_parts && (!bases || !read_off || !n_reads)) || !params) return fail_arg("null argument");
    GUARD({
        std::vector<mtsv::Batch::HostPart> parts((size_t)n_parts);
        for (int k = 0; k < n_parts; k++) {
            if (n_reads[k] && !read_off[k]) throw std::runtime_error("arg: null read_off");
            parts[(size_t)k] = mtsv::Batch::HostPart{bases[k], read_off[k], n_reads[k]};
        }
        b->impl.run_host_parts(parts.data(), n_parts, *params);
    })
}

int mtsv_batch_stats_get(const mtsv_batch* b, mtsv_batch_stats* st) {
    if (!b || !st) return fail_arg("null argument");
    *st = b->impl.stats;
    return MTSV_OK;
}

int mtsv_batch_set_taxa_report(mtsv_batch* b, int on) {
    if (!b) return fail_arg("null argument");
    GUARD(b->impl.set_taxa_report(on != 0))
}

int mtsv_batch_taxa_report(mtsv_batch* b, mtsv_taxon_stats** rows, uint64_t* n_rows, uint64_t* total_reads, float* device_ms, int reset) {
    if (!b || !rows || !n_rows || !total_reads) return fail_arg("null argument");
    GUARD({
        std::vector<mtsv_taxon_stats> r;
        float ms = 0;
        b->impl.taxa_report(r, total_reads, &ms, reset != 0);
        auto* out = (mtsv_taxon_stats*)malloc(std::max<size_t>(r.size(), 1) * sizeof(mtsv_taxon_stats));
        if (!out) throw std::bad_alloc();
        if (!r.empty()) memcpy(out, r.data(), r.size() * sizeof(mtsv_taxon_stats));
        *rows = out;
        *n_rows = r.size();
        if (device_ms) *device_ms = ms;
    })
}

int mtsv_batch_set_match_flags(mtsv_batch* b, int mode) {
    if (!b) return fail_arg("null argument");
    GUARD(b->impl.set_match_flags(mode))
}

int mtsv_batch_match_flags(mtsv_batch* b, uint64_t** words, uint64_t* n_reads, uint64_t* n_matched) {
    if (!b || !words || !n_reads || !n_matched) return fail_arg("null argument");
    GUARD({
        std::vector<uint64_t> w;
        b->impl.match_flags(w, n_reads, n_matched);
        auto* out = (uint64_t*)malloc(w.size() * sizeof(uint64_t));
        if (!out) throw std::bad_alloc();
        memcpy(out, w.data(), w.size() * sizeof(uint64_t));
        *words = out;
    })
}

int mtsv_batch_take_reads(mtsv_batch* dst, mtsv_batch* src, int keep, uint64_t* n_kept, uint64_t* bases_kept, float* device_ms) {
    if (!dst || !src || !n_kept || !bases_kept) return fail_arg("null argument");
    GUARD(dst->impl.take_reads(src->impl, keep, n_kept, bases_kept, device_ms))
}

int mtsv_batch_copy_reads(mtsv_batch* dst, mtsv_batch* src, float* device_ms) {
    if (!dst || !src) return fail_arg("null argument");
    GUARD(dst->impl.copy_reads(src->impl, device_ms))
}

int mtsv_batch_place_hits(mtsv_batch* b, const mtsv_hit* hits, uint64_t n_hits, mtsv_placement** out, uint64_t* n_out, uint32_t** ops, uint64_t* n_ops_total,
                          float* device_ms) {
    if (!b || !out || !n_out || !ops || !n_ops_total) return fail_arg("null argument");
    GUARD(b->impl.place_hits(hits, n_hits, out, n_out, ops, n_ops_total, device_ms))
}

int mtsv_batch_merge_runs(mtsv_batch* dst, mtsv_batch* const* srcs, int n_srcs, float* device_ms) {
    if (!dst || (n_srcs > 0 && !srcs)) return fail_arg("null argument");
    GUARD({
        std::vector<mtsv::Batch*> s;
        for (int k = 0; k < n_srcs; k++) {
            if (!srcs[k]) throw std::runtime_error("arg: null source workspace");
            s.push_back(&srcs[k]->impl);
        }
        dst->impl.merge_runs(s.data(), n_srcs, device_ms);
    })
}

int mtsv_batch_read_map(mtsv_batch* b, uint64_t** map, uint64_t* n_reads) {
    if (!b || !map || !n_reads) return fail_arg("null argument");
    GUARD({
        std::vector<uint64_t> m;
        b->impl.read_map(m);
        auto* out = (uint64_t*)malloc(std::max<size_t>(m.size(), 1) * sizeof(uint64_t));
        if (!out) throw std::bad_alloc();
        if (!m.empty()) memcpy(out, m.data(), m.size() * sizeof(uint64_t));
        *map = out;
        *n_reads = m.size();
    })
}

int mtsv_batch_download_reads(mtsv_batch* b, uint8_t** codes, uint64_t** read_off, uint64_t* n_reads) {
    if (!b || !codes || !read_off || !n_reads) return fail_arg("null argument");
    GUARD({
        std::vector<uint8_t> c;
        std::vector<uint64_t> o;
        b->impl.download_reads(c, o);
        auto* oc = (uint8_t*)malloc(std::max<size_t>(c.size(), 1));
        auto* oo = (uint64_t*)malloc(o.size() * sizeof(uint64_t));
        if (!oc || !oo) {
            free(oc);
            free(oo);
            throw std::bad_alloc();
        }
        if (!c.empty()) memcpy(oc, c.data(), c.size());
        memcpy(oo, o.data(), o.size() * sizeof(uint64_t));
        *codes = oc;
        *read_off = oo;
        *n_reads = o.size() - 1;
    })
}

int mtsv_merge_taxa_reports(const mtsv_taxon_stats* a, uint64_t n_a, const mtsv_taxon_stats* b, uint64_t n_b, mtsv_taxon_stats** out,
                            uint64_t* n_out) {
    if ((!a && n_a) || (!b && n_b) || !out || !n_out) return fail_arg("null argument");
    for (uint64_t i = 1; i < n_a; i++)
        if (a[i].tax_id <= a[i - 1].tax_id) return fail_arg("report rows are not ascending by tax_id");
    for (uint64_t i = 1; i < n_b; i++)
        if (b[i].tax_id <= b[i - 1].tax_id) return fail_arg("report rows are not ascending by tax_id");
    GUARD({
        auto* o = (mtsv_taxon_stats*)malloc(std::max<uint64_t>(n_a + n_b, 1) * sizeof(mtsv_taxon_stats));
        if (!o) throw std::bad_alloc();
        uint64_t i = 0, j = 0, n = 0;
        while (i < n_a || j < n_b) {
            if (j == n_b || (i < n_a && a[i].tax_id < b[j].tax_id)) o[n++] = a[i++];
            else if (i == n_a || b[j].tax_id < a[i].tax_id) o[n++] = b[j++];
            else {
                mtsv_taxon_stats r = a[i++];
                const mtsv_taxon_stats& q = b[j++];
                r.only_hit += q.only_hit;
                r.only_best += q.only_best;
                r.tied_best += q.tied_best;
                r.not_best += q.not_best;
                o[n++] = r;
            }
        }
        *out = o;
        *n_out = n;
    })
}

// write_taxa_report (collapse.rs:716-750)
int mtsv_format_taxa_report(const mtsv_taxon_stats* rows, uint64_t n_rows, uint64_t total_reads, char** out, uint64_t* out_len) {
    if ((!rows && n_rows) || !out || !out_len) return fail_arg("null argument");
    GUARD({
        std::string text = "taxid\tonly_hit\tonly_hit_pct\tonly_best\tonly_best_pct\ttied_best\ttied_best_pct\tnot_best\tnot_best_pct\ttotal_reads\ttotal_pct\n";
        const double denom = (double)std::max<uint64_t>(total_reads, 1);
        char line[512];
        for (uint64_t i = 0; i < n_rows; i++) {
            const mtsv_taxon_stats& s = rows[i];
            const uint64_t tot = s.only_hit + s.only_best + s.tied_best + s.not_best;
            snprintf(line, sizeof line, "%u\t%llu\t%.2f\t%llu\t%.2f\t%llu\t%.2f\t%llu\t%.2f\t%llu\t%.2f\n", s.tax_id,
                     (unsigned long long)s.only_hit, s.only_hit / denom * 100.0, (unsigned long long)s.only_best, s.only_best / denom * 100.0,
                     (unsigned long long)s.tied_best, s.tied_best / denom * 100.0, (unsigned long long)s.not_best, s.not_best / denom * 100.0,
                     (unsigned long long)tot, tot / denom * 100.0);
            text += line;
        }
        char* p = (char*)malloc(text.size() + 1);
        if (!p) throw std::bad_alloc();
        memcpy(p, text.c_str(), text.size() + 1);
        *out = p;
        *out_len = text.size();
    })
}

int mtsv_batch_set_assignments(mtsv_batch* b, int mode) {
    if (!b) return fail_arg("null argument");
    GUARD(b->impl.set_assignments(mode))
}

int mtsv_batch_download_assignments(mtsv_batch* b, mtsv_assignment** a, uint64_t* n, float* device_ms) {
    if (!b || !a || !n) return fail_arg("null argument");
    GUARD(b->impl.download_assignments((void**)a, n, device_ms, false))
}

static_assert(sizeof(mtsv_assignment) == 16 && sizeof(mtsv_assignment_gi) == 24, "the record sizes of the grains");
int mtsv_batch_set_assignment_grain(mtsv_batch* b, int grain) {
    if (!b) return fail_arg("null argument");
    GUARD(b->impl.set_assignment_grain(grain))
}

int mtsv_batch_download_assignments_gi(mtsv_batch* b, mtsv_assignment_gi** a, uint64_t* n, float* device_ms) {
    if (!b || !a || !n) return fail_arg("null argument");
    GUARD(b->impl.download_assignments((void**)a, n, device_ms, true))
}

// ---- mtsv_fold: assignment records accumulated across runs (fold.hip, k_fold.hip) ----
int mtsv_fold_create(int hip_device, int grain, mtsv_fold** out) {
    if (!out) return fail_arg("null argument");
    GUARD(*out = new mtsv_fold(hip_device, grain))
}

void mtsv_fold_free(mtsv_fold* f) { delete f; }

int mtsv_fold_reset(mtsv_fold* f, uint64_t n_reads) {
    if (!f) return fail_arg("null argument");
    GUARD(f->impl.reset(n_reads))
}

int mtsv_fold_add_run(mtsv_fold* f, mtsv_batch* src, float* device_ms) {
    if (!f || !src) return fail_arg("null argument");
    GUARD(f->impl.add_run(src->impl, device_ms))
}

int mtsv_fold_add_records(mtsv_fold* f, const void* records, uint64_t n, float* device_ms) {
    if (!f || (n && !records)) return fail_arg("null argument");
    GUARD(f->impl.add_records(records, n, device_ms))
}

int mtsv_fold_add_text(mtsv_fold* f, const char* hits, const uint64_t* line_off, const uint32_t* line_read, uint64_t n_lines, uint64_t* n_tokens,
                       uint64_t* n_records, float* device_ms) {
    if (!f || (n_lines && (!line_off || !line_read)) || (n_lines && line_off[n_lines] && !hits)) return fail_arg("null argument");
    GUARD(f->impl.add_text(hits, line_off, line_read, n_lines, n_tokens, n_records, device_ms))
}

int mtsv_fold_count(const mtsv_fold* f, uint64_t* n) {
    if (!f || !n) return fail_arg("null argument");
    *n = f->impl.n;
    return MTSV_OK;
}

int mtsv_fold_download(mtsv_fold* f, mtsv_assignment** a, uint64_t* n) {
    if (!f || !a || !n) return fail_arg("null argument");
    GUARD(f->impl.download((void**)a, n, false))
}

int mtsv_fold_download_gi(mtsv_fold* f, mtsv_assignment_gi** a, uint64_t* n) {
    if (!f || !a || !n) return fail_arg("null argument");
    GUARD(f->impl.download((void**)a, n, true))
}

int mtsv_fold_taxa_report(mtsv_fold* f, mtsv_taxon_stats** rows, uint64_t* n_rows, uint64_t* total_reads, float* device_ms) {
    if (!f || !rows || !n_rows || !total_reads) return fail_arg("null argument");
    GUARD({
        std::vector<mtsv_taxon_stats> r;
        f->impl.taxa_report(r, total_reads, device_ms);
        auto* out = (mtsv_taxon_stats*)malloc(std::max<size_t>(r.size(), 1) * sizeof(mtsv_taxon_stats));
        if (!out) throw std::bad_alloc();
        if (!r.empty()) memcpy(out, r.data(), r.size() * sizeof(mtsv_taxon_stats));
        *rows = out;
        *n_rows = r.size();
    })
}

int mtsv_fold_match_flags(mtsv_fold* f, uint64_t** words, uint64_t* n_reads, uint64_t* n_matched) {
    if (!f || !words || !n_reads || !n_matched) return fail_arg("null argument");
    GUARD({
        std::vector<uint64_t> w;
        f->impl.match_flags(w, n_reads, n_matched);
        auto* out = (uint64_t*)malloc(w.size() * sizeof(uint64_t));
        if (!out) throw std::bad_alloc();
        memcpy(out, w.data(), w.size() * sizeof(uint64_t));
        *words = out;
    })
}

// ---- mtsv_dupmap: identical reads binned once (dedup.hip, k_dedup.hip) ----
int mtsv_dupmap_create(int hip_device, mtsv_dupmap** out) {
    if (!out) return fail_arg("null argument");
    GUARD(*out = new mtsv_dupmap(hip_device))
}

void mtsv_dupmap_free(mtsv_dupmap* m) { delete m; }

int mtsv_batch_take_unique(mtsv_batch* dst, mtsv_batch* src, mtsv_dupmap* m, uint64_t* n_unique, uint64_t* bases_kept, float* device_ms) {
    if (!dst || !src || !m || !n_unique || !bases_kept) return fail_arg("null argument");
    GUARD(m->impl.take_unique(dst->impl, src->impl, n_unique, bases_kept, device_ms))
}

int mtsv_dupmap_download(const mtsv_dupmap* m, uint64_t** read, uint64_t** rep, uint64_t* n_reads, uint64_t* n_unique) {
    if (!m || !read || !rep || !n_reads || !n_unique) return fail_arg("null argument");
    GUARD({
        std::vector<uint64_t> a, b;
        m->impl.download(a, b);
        auto* oa = (uint64_t*)malloc(std::max<size_t>(a.size(), 1) * sizeof(uint64_t));
        auto* ob = (uint64_t*)malloc(std::max<size_t>(b.size(), 1) * sizeof(uint64_t));
        if (!oa || !ob) {
            free(oa);
            free(ob);
            throw std::bad_alloc();
        }
        if (!a.empty()) memcpy(oa, a.data(), a.size() * sizeof(uint64_t));
        if (!b.empty()) memcpy(ob, b.data(), b.size() * sizeof(uint64_t));
        *read = oa;
        *rep = ob;
        *n_reads = a.size();
        *n_unique = m->impl.valid ? m->impl.n_unique : 0;
    })
}

int mtsv_fold_expand(mtsv_fold* dst, mtsv_fold* src, const mtsv_dupmap* m, float* device_ms) {
    if (!dst || !src || !m) return fail_arg("null argument");
    GUARD(m->impl.expand(dst->impl, src->impl, device_ms))
}

// ---- taxonomy, per-read LCA and clade report (taxonomy.cpp, lca.hip, k_lca.hip) ----
int mtsv_taxonomy_load(const char* nodes_dmp, mtsv_taxonomy** out) {
    if (!nodes_dmp || !out) return fail_arg("null argument");
    GUARD(*out = new mtsv_taxonomy{Taxonomy::load(nodes_dmp)})
}

void mtsv_taxonomy_free(mtsv_taxonomy* tx) { delete tx; }

int mtsv_taxonomy_info(const mtsv_taxonomy* tx, mtsv_taxonomy_info_t* info) {
    if (!tx || !info) return fail_arg("null argument");
    info->n_nodes = tx->impl.ids.size();
    info->n_implied_roots = tx->impl.implied.size();
    info->n_ranks = (uint32_t)tx->impl.rank_names.size();
    info->max_depth = tx->impl.max_depth;
    return MTSV_OK;
}

int mtsv_taxonomy_parent(const mtsv_taxonomy* tx, uint32_t tax_id, uint32_t* parent, uint32_t* rank) {
    if (!tx || !parent || !rank) return fail_arg("null argument");
    (void)tx->impl.lookup(tax_id, parent, rank);
    return MTSV_OK;
}

const char* mtsv_taxonomy_rank_name(const mtsv_taxonomy* tx, uint32_t rank) { return tx ? tx->impl.rank_name(rank) : "-"; }

static_assert(sizeof(mtsv_clade_stats) == 32, "the clade row");
int mtsv_fold_lca(mtsv_fold* f, const mtsv_taxonomy* tx, uint32_t edit_slack, mtsv_fold* out, mtsv_clade_stats** rows, uint64_t* n_rows,
                  uint64_t* total_reads, float* device_ms) {
    if (!f || !tx) return fail_arg("null argument");
    if (rows && (!n_rows || !total_reads)) return fail_arg("rows without n_rows or total_reads");
    GUARD({
        std::vector<mtsv_clade_stats> r;
        mtsv_clade_stats* mem = nullptr;
        f->impl.lca(tx->impl, edit_slack, out ? &out->impl : nullptr, rows ? &r : nullptr, total_reads, device_ms);
        if (rows) {
            mem = (mtsv_clade_stats*)malloc(std::max<size_t>(r.size(), 1) * sizeof(mtsv_clade_stats));
            if (!mem) throw std::bad_alloc();
            if (!r.empty()) memcpy(mem, r.data(), r.size() * sizeof(mtsv_clade_stats));
            *rows = mem;
            *n_rows = r.size();
        }
    })
}

// ---- abundance by expectation-maximisation (abund.hip, k_abund.hip, abund_rows.hpp) ----
int mtsv_fold_abundance(mtsv_fold* f, const uint32_t* w, uint32_t n_w, uint32_t edit_slack, uint32_t max_iters, uint64_t tol, mtsv_fold* out,
                        mtsv_abundance_row** rows, uint64_t* n_rows, mtsv_abundance_info* info, float* device_ms) {
    if (!f || !w) return fail_arg("null argument");
    if (rows && !n_rows) return fail_arg("rows without n_rows");
    GUARD({
        std::vector<mtsv_abundance_row> r;
        f->impl.abundance(w, n_w, edit_slack, max_iters, tol, out ? &out->impl : nullptr, rows ? &r : nullptr, info, device_ms);
        if (rows) {
            *rows = malloc_copy(r);
            *n_rows = r.size();
        }
    })
}

int mtsv_abundance_weights(double q, uint32_t n_w, uint32_t* w) {
    if (!w) return fail_arg("null argument");
    GUARD(abundance_weights(q, n_w, w))
}

int mtsv_format_abundance(const mtsv_abundance_row* rows, uint64_t n_rows, const mtsv_abundance_info* info, char** out, uint64_t* out_len) {
    if ((!rows && n_rows) || !info || !out || !out_len) return fail_arg("null argument");
    GUARD({
        const std::string text = format_abundance(rows, n_rows, info);
        char* p = (char*)malloc(text.size() + 1);
        if (!p) throw std::bad_alloc();
        memcpy(p, text.c_str(), text.size() + 1);
        *out = p;
        *out_len = text.size();
    })
}

// ---- read pairs: the mates' records joined (pair.hip, k_pair.hip) ----
static_assert(sizeof(mtsv_pair_stats) == 40, "the pair stats");
int mtsv_fold_pair(mtsv_fold* f, int mode, uint32_t max_insert, uint32_t unpaired_edits, mtsv_fold* out, mtsv_pair_stats* stats, float* device_ms) {
    if (!f || !out) return fail_arg("null argument");
    GUARD(f->impl.pair(mode, max_insert, unpaired_edits, &out->impl, stats, device_ms))
}

// ---- coverage per reference sequence (cover.hip, k_cover.hip, cover_refs.hpp) ----
static_assert(sizeof(mtsv_ref_coverage) == 48, "the coverage row");
int mtsv_coverage_create(int hip_device, mtsv_coverage** out) {
    if (!out) return fail_arg("null argument");
    GUARD(*out = new mtsv_coverage(hip_device))
}

void mtsv_coverage_free(mtsv_coverage* c) { delete c; }

int mtsv_coverage_add_refs(mtsv_coverage* c, const uint32_t* tax_id, const uint32_t* gi, const uint64_t* length, uint64_t n) {
    if (!c || (n && (!tax_id || !gi || !length))) return fail_arg("null argument");
    GUARD(c->impl.add_refs(CoverRefs::normalise(tax_id, gi, length, n)))
}

int mtsv_coverage_add_index(mtsv_coverage* c, const mtsv_index* ix) {
    if (!c || !ix) return fail_arg("null argument");
    GUARD({
        const std::vector<Bin>& bins = ix->host.bins;
        std::vector<uint32_t> tax(bins.size()), gi(bins.size());
        std::vector<uint64_t> len(bins.size());
        for (size_t k = 0; k < bins.size(); k++) {
            tax[k] = bins[k].tax_id;
            gi[k] = bins[k].gi;
            len[k] = bins[k].end >= bins[k].start ? bins[k].end - bins[k].start : 0;
        }
        c->impl.add_refs(CoverRefs::normalise(tax.data(), gi.data(), len.data(), bins.size()));
    })
}

int mtsv_coverage_reset(mtsv_coverage* c) {
    if (!c) return fail_arg("null argument");
    GUARD(c->impl.reset())
}

int mtsv_coverage_add_fold(mtsv_coverage* c, mtsv_fold* f, const uint32_t* read_len, uint64_t n_reads, uint32_t edit_slack, float* device_ms) {
    if (!c || !f || !read_len) return fail_arg("null argument");
    GUARD(c->impl.add_fold(f->impl, read_len, n_reads, edit_slack, device_ms))
}

int mtsv_coverage_rows(mtsv_coverage* c, mtsv_ref_coverage** rows, uint64_t* n_rows, float* device_ms) {
    if (!c || !rows || !n_rows) return fail_arg("null argument");
    GUARD({
        std::vector<mtsv_ref_coverage> r;
        c->impl.rows(r, device_ms);
        auto* mem = (mtsv_ref_coverage*)malloc(std::max<size_t>(r.size(), 1) * sizeof(mtsv_ref_coverage));
        if (!mem) throw std::bad_alloc();
        if (!r.empty()) memcpy(mem, r.data(), r.size() * sizeof(mtsv_ref_coverage));
        *rows = mem;
        *n_rows = r.size();
    })
}

int mtsv_format_coverage_report(const mtsv_ref_coverage* rows, uint64_t n_rows, char** out, uint64_t* out_len) {
    if ((!rows && n_rows) || !out || !out_len) return fail_arg("null argument");
    GUARD({
        std::string text = "taxid\tgi\tlength\treads\talignments\taligned_bases\tdepth\tcovered_bases\tbreadth_pct\n";
        char line[320];
        auto put = [&](uint32_t tax_id, const char* gi, uint64_t length, uint64_t reads, uint64_t alignments, uint64_t bases, uint64_t covered) {
            const double depth = length ? (double)bases / (double)length : 0.0, breadth = length ? (double)covered / (double)length * 100.0 : 0.0;
            snprintf(line, sizeof line, "%u\t%s\t%llu\t%llu\t%llu\t%llu\t%.2f\t%llu\t%.2f\n", tax_id, gi, (unsigned long long)length, (unsigned long long)reads,
                     (unsigned long long)alignments, (unsigned long long)bases, depth, (unsigned long long)covered, breadth);
            text += line;
        };
        for (uint64_t i = 0; i < n_rows;) {
            uint64_t j = i, sum[5] = {0, 0, 0, 0, 0};
            bool any = false;
            for (; j < n_rows && rows[j].tax_id == rows[i].tax_id; j++) {
                const mtsv_ref_coverage& s = rows[j];
                const uint64_t v[5] = {s.length, s.reads, s.alignments, s.aligned_bases, s.covered_bases};
                for (int k = 0; k < 5; k++) sum[k] += v[k];
                if (!s.alignments) continue;
                any = true;
                char gi[16];
                snprintf(gi, sizeof gi, "%u", s.gi);
                put(s.tax_id, gi, s.length, s.reads, s.alignments, s.aligned_bases, s.covered_bases);
            }
            if (any) put(rows[i].tax_id, "*", sum[0], sum[1], sum[2], sum[3], sum[4]);
            i = j;
        }
        char* p = (char*)malloc(text.size() + 1);
        if (!p) throw std::bad_alloc();
        memcpy(p, text.c_str(), text.size() + 1);
        *out = p;
        *out_len = text.size();
    })
}

// ---- pileup per reference position (pile.hip, k_pile.hip, pile_refs.hpp) ----
static_assert(sizeof(mtsv_pile_site) == 48, "the pileup row");
int mtsv_pileup_create(int hip_device, const uint32_t* taxa, uint64_t n_taxa, mtsv_pileup** out) {
    if (!out || (n_taxa && !taxa)) return fail_arg("null argument");
    GUARD(*out = new mtsv_pileup(hip_device, taxa, n_taxa))
}

void mtsv_pileup_free(mtsv_pileup* p) { delete p; }

int mtsv_pileup_reset(mtsv_pileup* p) {
    if (!p) return fail_arg("null argument");
    GUARD(p->impl.reset())
}

int mtsv_pileup_add_run(mtsv_pileup* p, mtsv_batch* b, const mtsv_hit* hits, uint64_t n_hits, uint32_t edit_slack, uint64_t* n_piled, uint64_t* n_skipped,
                        float* device_ms) {
    if (!p || !b) return fail_arg("null argument");
    GUARD(p->impl.add_run(b->impl, hits, n_hits, edit_slack, n_piled, n_skipped, device_ms))
}

int mtsv_pileup_info(const mtsv_pileup* p, mtsv_pileup_info_t* info) {
    if (!p || !info) return fail_arg("null argument");
    GUARD(p->impl.info(info))
}

int mtsv_pileup_download(mtsv_pileup* p, uint32_t tax_id, uint32_t gi, uint32_t** counts, uint8_t** ref, uint64_t* n_slots) {
    if (!p || !counts || !ref || !n_slots) return fail_arg("null argument");
    GUARD({
        std::vector<uint32_t> c;
        std::vector<uint8_t> r;
        p->impl.download(tax_id, gi, c, r);
        uint32_t* cm = malloc_copy(c);
        uint8_t* rm = nullptr;
        try {
            rm = malloc_copy(r);
        } catch (...) {
            free(cm);
            throw;
        }
        *counts = cm;
        *ref = rm;
        *n_slots = r.size();
    })
}

int mtsv_pileup_sites(mtsv_pileup* p, uint32_t min_depth, uint32_t min_alt, uint32_t min_alt_ppm, mtsv_pile_site** rows, uint64_t* n_rows, float* device_ms) {
    if (!p || !rows || !n_rows) return fail_arg("null argument");
    GUARD({
        std::vector<mtsv_pile_site> r;
        p->impl.sites(min_depth, min_alt, min_alt_ppm, r, device_ms);
        *rows = malloc_copy(r);
        *n_rows = r.size();
    })
}

int mtsv_format_variants(const mtsv_pile_site* rows, uint64_t n_rows, char** out, uint64_t* out_len) {
    if ((!rows && n_rows) || !out || !out_len) return fail_arg("null argument");
    GUARD({
        std::string text = "taxid\tgi\tpos\tref\tdepth\tmatch\tA\tC\tG\tT\tN\tdel\tins\n";
        char line[256];
        for (uint64_t i = 0; i < n_rows; i++) {
            const mtsv_pile_site& s = rows[i];
            uint64_t depth = 0;
            for (int c = 0; c < 7; c++) depth += s.n[c];
            snprintf(line, sizeof line, "%u\t%u\t%u\t%c\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", s.tax_id, s.gi, s.pos, s.ref < 5 ? "ACGTN"[s.ref] : '.',
                     (unsigned long long)depth, s.n[0], s.n[1], s.n[2], s.n[3], s.n[4], s.n[5], s.n[6], s.n[7]);
            text += line;
        }
        char* q = (char*)malloc(text.size() + 1);
        if (!q) throw std::bad_alloc();
        memcpy(q, text.c_str(), text.size() + 1);
        *out = q;
        *out_len = text.size();
    })
}

// ---- consensus from the pileup (cons.hip, k_cons.hip, cons_rows.hpp) ----
int mtsv_pileup_consensus(mtsv_pileup* p, uint32_t min_depth, uint32_t min_frac_ppm, uint32_t min_breadth_ppm, uint32_t fill, uint32_t line_width, char** fasta,
                          uint64_t* fasta_len, mtsv_cons_ref** rows, uint64_t* n_rows, float* device_ms) {
    if (!p || (fasta && !fasta_len) || (rows && !n_rows)) return fail_arg("null argument");
    GUARD({
        std::vector<char> text;
        std::vector<mtsv_cons_ref> r;
        p->impl.consensus(min_depth, min_frac_ppm, min_breadth_ppm, fill, line_width, fasta ? &text : nullptr, r, device_ms);
        char* tm = fasta ? malloc_copy(text) : nullptr;
        if (rows) {
            try {
                *rows = malloc_copy(r);
            } catch (...) {
                free(tm);
                throw;
            }
        }
        if (n_rows) *n_rows = r.size();
        if (fasta) {
            *fasta = tm;
            *fasta_len = text.size();
        }
    })
}

int mtsv_format_consensus_stats(const mtsv_cons_ref* rows, uint64_t n_rows, char** out, uint64_t* out_len) {
    if ((!rows && n_rows) || !out || !out_len) return fail_arg("null argument");
    GUARD({
        const std::string text = format_consensus_stats(rows, n_rows);
        char* q = (char*)malloc(text.size() + 1);
        if (!q) throw std::bad_alloc();
        memcpy(q, text.c_str(), text.size() + 1);
        *out = q;
        *out_len = text.size();
    })
}

int mtsv_pileup_add_counts(mtsv_pileup* p, uint32_t tax_id, uint32_t gi, uint32_t first_slot, uint64_t n_slots, const uint32_t* counts, uint64_t n_hits) {
    if (!p || (n_slots && !counts)) return fail_arg("null argument");
    GUARD(p->impl.add_counts(tax_id, gi, first_slot, n_slots, counts, n_hits))
}

int mtsv_format_clade_report(const mtsv_clade_stats* rows, uint64_t n_rows, uint64_t total_reads, const mtsv_taxonomy* tx, char** out,
                             uint64_t* out_len) {
    if ((!rows && n_rows) || !out || !out_len) return fail_arg("null argument");
    GUARD({
        std::string text = "taxid\tparent\trank\tdepth\tdirect\tdirect_pct\tclade\tclade_pct\n";
        const double denom = (double)std::max<uint64_t>(total_reads, 1);
        char line[256];
        for (uint64_t i = 0; i < n_rows; i++) {
            const mtsv_clade_stats& s = rows[i];
            snprintf(line, sizeof line, "%u\t%u\t", s.tax_id, s.parent_tax_id);
            text += line;
            text += tx ? tx->impl.rank_name(s.rank) : "-";
            snprintf(line, sizeof line, "\t%u\t%llu\t%.2f\t%llu\t%.2f\n", s.depth, (unsigned long long)s.direct, s.direct / denom * 100.0,
                     (unsigned long long)s.clade, s.clade / denom * 100.0);
            text += line;
        }
        char* p = (char*)malloc(text.size() + 1);
        if (!p) throw std::bad_alloc();
        memcpy(p, text.c_str(), text.size() + 1);
        *out = p;
        *out_len = text.size();
    })
}

// ---- the result lines written on the device (text.hip, k_text.hip) ----
int mtsv_fold_format_text(mtsv_fold* f, const char* ids, const uint64_t* id_off, uint64_t n_reads, char** text, uint64_t* len, float* device_ms) {
    if (!f || !ids || !id_off || !text || !len) return fail_arg("null argument");
    GUARD(f->impl.format_text(ids, id_off, n_reads, text, len, device_ms))
}

int mtsv_batch_format_text(mtsv_batch* b, const char* ids, const uint64_t* id_off, uint64_t n_reads, char** text, uint64_t* len, float* device_ms) {
    if (!b || !ids || !id_off || !text || !len) return fail_arg("null argument");
    GUARD(b->impl.format_text(ids, id_off, n_reads, text, len, device_ms))
}

int mtsv_batch_download(mtsv_batch* b, mtsv_hit** hits, uint64_t* n_hits) {
    if (!b || !hits || !n_hits) return fail_arg("null argument");
    GUARD(b->impl.download(hits, n_hits))
}

int mtsv_batch_set_verify_mode(mtsv_batch* b, int mode) {
    if (!b || (mode != MTSV_VERIFY_REFERENCE && mode != MTSV_VERIFY_EDIT_FIRST)) return fail_arg("bad verify mode");
    b->impl.verify_mode = mode;
    return MTSV_OK;
}

int mtsv_set_default_verify_mode(int mode) {
    if (mode != MTSV_VERIFY_REFERENCE && mode != MTSV_VERIFY_EDIT_FIRST) return fail_arg("bad verify mode");
    mtsv::g_default_verify_mode = mode;
    return MTSV_OK;
}

void mtsv_batch_free(mtsv_batch* b) { delete b; }

// Three lanes of up to 1 Mi reads each (MTSV_WORKSPACE_READS overrides): ~2.7 KB of HBM per workspace read.
uint64_t mtsv_bin_batch_workspace_reads(uint64_t n_reads) {
    uint64_t cap = 3ull << 20;
    if (const char* e = getenv("MTSV_WORKSPACE_READS")) cap = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    return std::min<uint64_t>(std::max<uint64_t>(n_reads, 1024), cap);
}

// One host batch (or a contiguous part of one) on one device, through the workspace kept for (device, slot).
// hold == nullptr: the hits come back in a pooled page-locked array (*hits, *n_hits).
// hold != nullptr: the hits stay in HBM, *n_hits says how many, and `hold` keeps the workspace locked until the
// caller has fetched them with impl.download_into (mtsv_bin_batch_multi: every part straight into its extent of
// one result array, once all the counts are known).
struct HeldWorkspace {
    std::unique_lock<std::mutex> lk;
    mtsv_batch* b = nullptr;
};
static void bin_batch_on(mtsv_index* ix, int hip_device, int slot, const uint8_t* bases, const uint64_t* read_off, uint64_t n_reads,
                         uint64_t read_base, const mtsv_params& params, mtsv_hit** hits, uint64_t* n_hits, HeldWorkspace* hold = nullptr) {
    if (hip_device < 0) throw std::runtime_error("arg: hip_device must name a GPU: this library has no CPU path");
    uint32_t flags = MTSV_DEV_DEFAULT;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        if (ix->dev.count(hip_device)) flags = ix->dev[hip_device]->flags;
    }
    if (int rc = mtsv_index_to_device(ix, hip_device, flags); rc != MTSV_OK) throw std::runtime_error(g_err);
    mtsv_cached_workspace* ws;
    DeviceIndex* di;
    {
        std::lock_guard<std::mutex> lk(ix->mu);
        auto& slot_ws = ix->cached_batch[{hip_device, slot}];
        if (!slot_ws) slot_ws = std::make_unique<mtsv_cached_workspace>();
        ws = slot_ws.get();
        di = device_index(ix, hip_device);
    }
    std::unique_lock<std::mutex> wl(ws->mu);
    // Workspace for ranges of a bounded number of reads: larger host batches stream through it (run_host),
    // which bounds the workspace (~2.7 KB of HBM per read) and overlaps the copies with compute.
    const uint64_t nb = n_reads ? read_off[n_reads] - read_off[0] : 0;
    const uint64_t slice_reads = mtsv_bin_batch_workspace_reads(n_reads);
    const uint64_t slice_bases = n_reads > slice_reads
                                     ? std::max<uint64_t>(1 << 16, (uint64_t)((double)nb / (double)n_reads * (double)slice_reads * 1.25) + 4096)
                                     : std::max<uint64_t>(nb, 1 << 16);
    if (!ws->b || ws->b->impl.max_reads < slice_reads || ws->b->impl.max_bases < slice_bases) {
        delete ws->b;
        ws->b = nullptr;
        ws->b = new mtsv_batch(ix, di, slice_reads, slice_bases, 0);
    }
    ws->b->impl.keep_on_device = hold != nullptr;
    try {
        ws->b->impl.run_host(bases, read_off, n_reads, params, read_base);
    } catch (...) {
        ws->b->impl.keep_on_device = false;
        throw;
    }
    ws->b->impl.keep_on_device = false;
    if (hold) {
        *n_hits = ws->b->impl.total_hits;
        hold->b = ws->b;
        hold->lk = std::move(wl);
    } else {
        ws->b->impl.download(hits, n_hits);
    }
}

int mtsv_bin_batch(mtsv_index* ix, int hip_device, const uint8_t* bases, const uint64_t* read_off, uint64_t n_reads,
                   const mtsv_params* params, mtsv_hit** hits, uint64_t* n_hits) {
    if (!ix || !read_off || !params || !hits || !n_hits) return fail_arg("null argument");
    if (hip_device < 0) return fail_arg("hip_device must name a GPU: this library has no CPU path");
    GUARD(bin_batch_on(ix, hip_device, 0, bases, read_off, n_reads, 0, *params, hits, n_hits))
}


// Mode A of SURVEY 8(e): index replicated, reads in contiguous blocks, host concat.
int mtsv_bin_batch_multi(mtsv_index* ix, const int* devices, int n_devices, const uint8_t* bases, const uint64_t* read_off,
                         uint64_t n_reads, const mtsv_params* params, mtsv_hit** hits, uint64_t* n_hits) {
    if (!ix || !devices || n_devices < 1 || !read_off || !params || !hits || !n_hits) return fail_arg("null argument");
    if (n_devices == 1) {
        GUARD(bin_batch_on(ix, devices[0], 0, bases, read_off, n_reads, 0, *params, hits, n_hits))
    }
    // Two phases.  Every part runs on its device and leaves its hits in HBM; once all the counts are known, every part
    // copies its hits straight into its extent of ONE pooled page-locked array (no host-side concatenation: at 100 M
    // reads that was 3 GB of memcpy behind the slowest device).  The call returns when the slowest device has: a caller
    // that wants no such barrier runs mtsv_bin_batch per device from its own threads (what mtsv-binner --devices does).
    std::vector<HeldWorkspace> held(n_devices);
    std::vector<uint64_t> cnt(n_devices, 0);
    mtsv_hit* out = nullptr;
    try {
        fork_join(n_devices, [&](int k) {
            const uint64_t a = n_reads * (uint64_t)k / n_devices, b = n_reads * (uint64_t)(k + 1) / n_devices;
            bin_batch_on(ix, devices[k], slot_of(devices, k), bases, read_off + a, b - a, a, *params, nullptr, &cnt[k], &held[k]);
        });
        uint64_t total = 0, cap = 0;
        for (auto c : cnt) total += c;
        out = pinned_hits_alloc(total, &cap);
        std::vector<uint64_t> at(n_devices + 1, 0);
        for (int k = 0; k < n_devices; k++) at[k + 1] = at[k] + cnt[k];
        fork_join(n_devices, [&](int k) {
            held[k].b->impl.download_into(out + at[k], cnt[k]);
            held[k].lk.unlock();
        });
        *hits = out;
        *n_hits = total;
        return MTSV_OK;
    } catch (const std::exception& e) {
        if (out) pinned_hits_release(out);
        return fail(e);
    }
}

// Mode B of SURVEY 8(e): one chunk of the database per entry, every chunk sees every read, the hit lists are
// merged per read (mtsv-collapse then keeps the smallest edit per (read, TaxId): collapse.rs:597-602 -- and so
// does mtsv_format_results on the merged list).
int mtsv_bin_batch_chunks(mtsv_index* const* chunks, const int* devices, int n_chunks, const uint8_t* bases,
                          const uint64_t* read_off, uint64_t n_reads, const mtsv_params* params, mtsv_hit** hits, uint64_t* n_hits) {
    if (!chunks || !devices || n_chunks < 1 || !read_off || !params || !hits || !n_hits) return fail_arg("null argument");
    for (int k = 0; k < n_chunks; k++)
        if (!chunks[k]) return fail_arg("null chunk index");
    std::vector<mtsv_hit*> parts(n_chunks, nullptr);
    std::vector<uint64_t> cnt(n_chunks, 0);
    try {
        fork_join(n_chunks, [&](int k) {
            // distinct index handles own distinct workspaces: slot 0 each
            bin_batch_on(chunks[k], devices[k], 0, bases, read_off, n_reads, 0, *params, &parts[k], &cnt[k]);
        });
        if (n_chunks == 1) {
            *hits = parts[0];
            *n_hits = cnt[0];
            return MTSV_OK;
        }
        uint64_t total = 0, cap = 0;
        for (auto c : cnt) total += c;
        mtsv_hit* out = pinned_hits_alloc(total, &cap);
        // k-way merge by read, chunk order within a read; read ranges in parallel
        const int T = (int)std::min<uint64_t>(8, std::max<uint64_t>(1, total >> 16));
        auto lower = [&](int k, uint64_t r) {  // first hit of part k with read >= r
            return (uint64_t)(std::lower_bound(parts[k], parts[k] + cnt[k], r, [](const mtsv_hit& h, uint64_t v) { return h.read < v; }) - parts[k]);
        };
        fork_join(T, [&](int t) {
            const uint64_t r0 = n_reads * (uint64_t)t / T, r1 = n_reads * (uint64_t)(t + 1) / T;
            std::vector<uint64_t> pos(n_chunks), end(n_chunks);
            uint64_t o = 0;
            for (int k = 0; k < n_chunks; k++) {
                pos[k] = lower(k, r0);
                end[k] = t + 1 == T ? cnt[k] : lower(k, r1);
                o += pos[k];
            }
            for (;;) {
                uint64_t r = ~0ull;
                for (int k = 0; k < n_chunks; k++)
                    if (pos[k] < end[k]) r = std::min(r, parts[k][pos[k]].read);
                if (r == ~0ull) break;
                for (int k = 0; k < n_chunks; k++)
                    while (pos[k] < end[k] && parts[k][pos[k]].read == r) out[o++] = parts[k][pos[k]++];
            }
        });
        release_parts(parts);
        *hits = out;
        *n_hits = total;
        return MTSV_OK;
    } catch (const std::exception& e) {
        release_parts(parts);
        return fail(e);
    }
}

void mtsv_hits_free(mtsv_hit* hits) {
    if (hits && !mtsv::pinned_hits_release(hits)) free(hits);
}
void mtsv_free(void* p) {  // (arrays of the pinned pool go back to it)
    if (p && !mtsv::pinned_hits_release(p)) free(p);
}

void* mtsv_host_alloc(size_t bytes) {
    void* p = mtsv::host_pinned_alloc(bytes);
    if (!p) g_err = "device: page-locked allocation of " + std::to_string(bytes) + " bytes failed (no HIP device?)";
    return p;
}
void mtsv_host_free(void* p) { mtsv::host_pinned_free(p); }
int mtsv_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return fail_arg("null argument");
    if (!mtsv::host_pinned_register(p, bytes)) {
        g_err = "device: the memory could not be page-locked (no HIP device, or the range is already registered)";
        return MTSV_E_DEVICE;
    }
    return MTSV_OK;
}
int mtsv_host_unregister(void* p) {
    if (!p) return fail_arg("null argument");
    if (!mtsv::host_pinned_unregister(p)) {
        g_err = "device: not a registered range";
        return MTSV_E_DEVICE;
    }
    return MTSV_OK;
}

// ---- write_assignments (src/binner.rs:310-379) ------------------------------------------------
// the text grows in a malloc'd buffer that is handed to the caller as it is; numbers are written digit by
// digit (snprintf per TaxID cost more than everything else on the result side of mtsv-binner)
namespace {
struct Text {
    char* p = nullptr;
    uint64_t n = 0, cap = 0;
    ~Text() { free(p); }
    void room(uint64_t more) {
        if (n + more <= cap) return;
        const uint64_t ncap = std::max<uint64_t>(n + more, cap + cap / 2 + (1 << 16));
        char* q = (char*)realloc(p, ncap);
        if (!q) throw std::bad_alloc();
        p = q;
        cap = ncap;
    }
    void put(uint64_t v) {  // decimal, as %u / %llu
        char tmp[20];
        int k = 0;
        do {
            tmp[k++] = (char)('0' + v % 10);
            v /= 10;
        } while (v);
        while (k) p[n++] = tmp[--k];
    }
};
}  // namespace

int mtsv_format_results(const mtsv_hit* hits, uint64_t n_hits, const char* ids, const uint64_t* id_off, uint64_t n_reads,
                        int long_format, char** out, uint64_t* out_len) {
    if ((!hits && n_hits) || !ids || !id_off || !out || !out_len) return fail_arg("null argument");
    GUARD({
        Text buf;
        struct Item {
            uint32_t tax, gi;
            uint64_t off;
            uint32_t edit;
        };
        std::vector<Item> items;
        uint64_t i = 0;
        while (i < n_hits) {
            uint64_t r = hits[i].read;
            if (r >= n_reads) throw std::runtime_error("arg: hit refers to a read outside the batch");
            uint64_t j = i;
            items.clear();
            for (; j < n_hits && hits[j].read == r; j++) {
                const mtsv_hit& h = hits[j];
                bool found = false;
                for (auto& it : items) {
                    bool same = long_format ? (it.tax == h.tax_id && it.gi == h.gi && it.off == h.offset) : it.tax == h.tax_id;
                    if (same) {
                        if (h.edit < it.edit) it.edit = h.edit;  // smallest edit per key (binner.rs:326-331,358-361)
                        found = true;
                        break;
                    }
                }
                if (!found) items.push_back(Item{h.tax_id, h.gi, h.offset, h.edit});
            }
            if (j < n_hits && hits[j].read < r) throw std::runtime_error("arg: hits are not ordered by read");
            if (long_format)
                std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
                    if (a.tax != b.tax) return a.tax < b.tax;
                    if (a.gi != b.gi) return a.gi < b.gi;
                    if (a.off != b.off) return a.off < b.off;
                    return a.edit < b.edit;
                });
            else
                std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
                    if (a.tax != b.tax) return a.tax < b.tax;
                    return a.edit < b.edit;
                });
            const uint64_t id_len = strnlen(ids + id_off[r], id_off[r + 1] - id_off[r]);
            buf.room(id_len + 2 + items.size() * 56 + 1);  // "tax-gi-offset=edit," is at most 10 + 1 + 10 + 1 + 20 + 1 + 10 + 1 characters
            memcpy(buf.p + buf.n, ids + id_off[r], id_len);
            buf.n += id_len;
            buf.p[buf.n++] = ':';
            bool first = true;
            for (auto& it : items) {
                if (!first) buf.p[buf.n++] = ',';
                first = false;
                buf.put(it.tax);
                if (long_format) {  // "%u-%u-%llu=%u"
                    buf.p[buf.n++] = '-';
                    buf.put(it.gi);
                    buf.p[buf.n++] = '-';
                    buf.put(it.off);
                }
                buf.p[buf.n++] = '=';
                buf.put(it.edit);
            }
            buf.p[buf.n++] = '\n';
            i = j;
        }
        buf.room(1);
        buf.p[buf.n] = 0;
        *out = buf.p;
        *out_len = buf.n;
        buf.p = nullptr;  // the caller's now (mtsv_free)
    })
}

// the same lines from the device's assignments: already one per (read, TaxID), smallest edit, ascending
int mtsv_format_assignments(const mtsv_assignment* a, uint64_t n, const char* ids, const uint64_t* id_off, uint64_t n_reads, char** out,
                            uint64_t* out_len) {
    if ((!a && n) || !ids || !id_off || !out || !out_len) return fail_arg("null argument");
    GUARD({
        Text buf;
        uint64_t i = 0;
        while (i < n) {
            const uint64_t r = a[i].read;
            if (r >= n_reads) throw std::runtime_error("arg: assignment refers to a read outside the batch");
            if (i && r < a[i - 1].read) throw std::runtime_error("arg: assignments are not ordered by read");
            uint64_t j = i;
            while (j < n && a[j].read == r) j++;
            const uint64_t id_len = strnlen(ids + id_off[r], id_off[r + 1] - id_off[r]);
            buf.room(id_len + 2 + (j - i) * 22 + 1);  // "tax=edit," is at most 10 + 1 + 10 + 1 characters
            memcpy(buf.p + buf.n, ids + id_off[r], id_len);
            buf.n += id_len;
            buf.p[buf.n++] = ':';
            for (uint64_t k = i; k < j; k++) {
                if (k != i) buf.p[buf.n++] = ',';
                buf.put(a[k].tax_id);
                buf.p[buf.n++] = '=';
                buf.put(a[k].edit);
            }
            buf.p[buf.n++] = '\n';
            i = j;
        }
        buf.room(1);
        buf.p[buf.n] = 0;
        *out = buf.p;
        *out_len = buf.n;
        buf.p = nullptr;  // the caller's now (mtsv_free)
    })
}

// one line per placement: READ_ID TAXID GI +|- START END EDIT CIGAR, tab-separated
int mtsv_format_placements(const mtsv_placement* pl, uint64_t n, const uint32_t* ops, const char* ids, const uint64_t* id_off, uint64_t n_reads, char** out,
                           uint64_t* out_len) {
    if ((!pl && n) || !ids || !id_off || !out || !out_len) return fail_arg("null argument");
    GUARD({
        Text buf;
        static const char kOp[] = "MIDNSHP=X";  // BAM's op codes
        for (uint64_t i = 0; i < n; i++) {
            const mtsv_placement& q = pl[i];
            if (q.read >= n_reads)
                throw std::runtime_error("arg: placement " + std::to_string(i) + " refers to read " + std::to_string(q.read) + ", outside the batch of " +
                                         std::to_string(n_reads));
            if (q.n_ops && !ops) throw std::runtime_error("arg: null argument");
            const uint64_t id_len = strnlen(ids + id_off[q.read], id_off[q.read + 1] - id_off[q.read]);
            buf.room(id_len + 5 * 11 + 4 + (uint64_t)q.n_ops * 11 + 2);  // five numbers and the strand, tabs; "len op" is at most 10 + 1 characters
            memcpy(buf.p + buf.n, ids + id_off[q.read], id_len);
            buf.n += id_len;
            buf.p[buf.n++] = '\t';
            buf.put(q.tax_id);
            buf.p[buf.n++] = '\t';
            buf.put(q.gi);
            buf.p[buf.n++] = '\t';
            buf.p[buf.n++] = q.strand ? '-' : '+';
            buf.p[buf.n++] = '\t';
            buf.put(q.ref_start);
            buf.p[buf.n++] = '\t';
            buf.put(q.ref_end);
            buf.p[buf.n++] = '\t';
            buf.put(q.edit);
            buf.p[buf.n++] = '\t';
            if (!q.n_ops) buf.p[buf.n++] = '*';
            for (uint32_t k = 0; k < q.n_ops; k++) {
                const uint32_t op = ops[q.ops_off + k];
                buf.put(op >> 4);
                buf.p[buf.n++] = (op & 15u) < 9 ? kOp[op & 15u] : '?';
            }
            buf.p[buf.n++] = '\n';
        }
        buf.room(1);
        buf.p[buf.n] = 0;
        *out = buf.p;
        *out_len = buf.n;
        buf.p = nullptr;  // the caller's now (mtsv_free)
    })
}

// the long lines from the device's wide assignments: already one per key of the grain, in the grain's order
int mtsv_format_assignments_gi(const mtsv_assignment_gi* a, uint64_t n, const char* ids, const uint64_t* id_off, uint64_t n_reads, char** out,
                               uint64_t* out_len) {
    if ((!a && n) || !ids || !id_off || !out || !out_len) return fail_arg("null argument");
    GUARD({
        Text buf;
        uint64_t i = 0;
        while (i < n) {
            const uint64_t r = a[i].read;
            if (r >= n_reads) throw std::runtime_error("arg: assignment refers to a read outside the batch");
            if (i && r < a[i - 1].read) throw std::runtime_error("arg: assignments are not ordered by read");
            uint64_t j = i;
            while (j < n && a[j].read == r) j++;
            const uint64_t id_len = strnlen(ids + id_off[r], id_off[r + 1] - id_off[r]);
            buf.room(id_len + 2 + (j - i) * 44 + 1);  // "tax-gi-offset=edit," is at most 10 + 1 + 10 + 1 + 10 + 1 + 10 + 1 characters
            memcpy(buf.p + buf.n, ids + id_off[r], id_len);
            buf.n += id_len;
            buf.p[buf.n++] = ':';
            for (uint64_t k = i; k < j; k++) {
                if (k != i) buf.p[buf.n++] = ',';
                buf.put(a[k].tax_id);
                buf.p[buf.n++] = '-';
                buf.put(a[k].gi);
                buf.p[buf.n++] = '-';
                buf.put(a[k].offset);
                buf.p[buf.n++] = '=';
                buf.put(a[k].edit);
            }
            buf.p[buf.n++] = '\n';
            i = j;
        }
        buf.room(1);
        buf.p[buf.n] = 0;
        *out = buf.p;
        *out_len = buf.n;
        buf.p = nullptr;  // the caller's now (mtsv_free)
    })
}

// ---- synthetic workloads -------------------------------------------------------

int mtsv_synth_index(uint64_t seed, uint32_t n_taxa, uint32_t gis_per_taxon, uint64_t seq_len, uint32_t occ_k,
                     uint64_t sa_s, int n_threads, mtsv_index** out) {
    if (!out || !n_taxa || !gis_per_taxon || seq_len < 64) return fail_arg("bad synthetic database shape");
    GUARD({
        const uint64_t nseq = (uint64_t)n_taxa * gis_per_taxon;
        std::vector<std::string> seqs(nseq);
        static const char ACGT[4] = {'A', 'C', 'G', 'T'};
        par_for(nseq, n_threads, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; i++) {
                SplitMix64 rng(mix(seed, i));
                std::string& s = seqs[i];
                s.resize(seq_len);
                for (uint64_t p = 0; p < seq_len;) {
                    uint64_t w = rng.next();
                    for (int k = 0; k < 32 && p < seq_len; k++, p++, w >>= 2) s[p] = ACGT[w & 3];
                }
            }
        });
        // 5% of every GI: a 1%-diverged copy of a segment of a GI of another taxon
        SplitMix64 rng(mix(seed, 0xC0FFEE));
        const uint64_t seg = std::max<uint64_t>(1, seq_len / 20);
        if (n_taxa > 1)
            for (uint64_t i = 0; i < nseq; i++) {
                uint64_t my_tax = i / gis_per_taxon;
                uint64_t src_tax = rng.below(n_taxa - 1);
                if (src_tax >= my_tax) src_tax++;
                uint64_t src = src_tax * gis_per_taxon + rng.below(gis_per_taxon);
                uint64_t sp = rng.below(seq_len - seg + 1), dp = rng.below(seq_len - seg + 1);
                for (uint64_t k = 0; k < seg; k++) {
                    char c = seqs[src][sp + k];
                    if (rng.chance(0.01)) c = ACGT[rng.below(4)];
                    seqs[i][dp + k] = c;
                }
            }
        // 0.1% of positions in runs of N of length 10..100
        for (uint64_t i = 0; i < nseq; i++) {
            uint64_t target = seq_len / 1000, placed = 0;
            while (placed < target) {
                uint64_t len = 10 + rng.below(91);
                if (len >= seq_len) break;
                uint64_t at = rng.below(seq_len - len);
                for (uint64_t k = 0; k < len; k++) seqs[i][at + k] = 'N';
                placed += len;
            }
        }
        // distinct TaxIDs / GIs
        std::vector<uint32_t> tax(nseq), gi(nseq);
        std::vector<uint32_t> taxids;
        while (taxids.size() < n_taxa) {
            uint32_t t = (uint32_t)rng.next();
            if (std::find(taxids.begin(), taxids.end(), t) == taxids.end()) taxids.push_back(t);
        }
        for (uint64_t i = 0; i < nseq; i++) {
            tax[i] = taxids[i / gis_per_taxon];
            gi[i] = (uint32_t)(mix(seed ^ 0x6D747376ull, i) | 1u) + (uint32_t)i;  // distinct enough; uniqueness not required
        }
        std::vector<SeqEntry> e(nseq);
        for (uint64_t i = 0; i < nseq; i++) e[i] = SeqEntry{tax[i], gi[i], (const uint8_t*)seqs[i].data(), seqs[i].size()};
        auto ix = std::make_unique<mtsv_index>();
        build_index(std::move(e), occ_k, sa_s, n_threads, ix->host, g_build_device);
        *out = ix.release();
    })
}

int mtsv_host_pack_threads(void) {
    if (getenv("MTSV_H2D_PLAIN")) return 0;
    const int n = mtsv::pack_threads();
    return n >= mtsv::kPackWorthwhile ? n : 0;
}

uint8_t mtsv_pack_bases(uint8_t* dst, const uint8_t* src, uint64_t first_offset, uint64_t n, uint8_t prev_code) {
    return mtsv::pack_chunk(dst, src, first_offset, n, prev_code);
}

int mtsv_synth_reads(const mtsv_index* ix, uint64_t seed, uint64_t n_reads, uint32_t read_len, uint8_t* bases,
                     uint64_t* read_off) {
    if (!ix || !bases || !read_off || read_len == 0) return fail_arg("null argument");
    const std::vector<uint8_t>& text = ix->host.text;
    if (text.size() < (uint64_t)read_len * 2 + 16) return fail_arg("index too small for this read length");
    GUARD({
        static const uint8_t ACGT[4] = {'A', 'C', 'G', 'T'};
        int threads = (int)std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
        const uint64_t span = text.size() - 1 - ((uint64_t)read_len + read_len / 4 + 8);
        for (uint64_t r = 0; r <= n_reads; r++) read_off[r] = r * read_len;
        par_for(n_reads, threads, [&](uint64_t lo, uint64_t hi) {
            std::vector<uint8_t> tmp(read_len);
            for (uint64_t r = lo; r < hi; r++) {
                SplitMix64 rng(mix(seed, r));
                uint8_t* dst = bases + r * read_len;
                if (rng.chance(0.10)) {  // no origin
                    for (uint32_t i = 0; i < read_len; i++) dst[i] = ACGT[rng.below(4)];
                    continue;
                }
                uint64_t p = rng.below(span);
                uint32_t i = 0;
                while (i < read_len) {
                    if (rng.chance(0.001)) {  // deletion from the read
                        p++;
                        continue;
                    }
                    if (rng.chance(0.001)) {  // insertion
                        tmp[i++] = ACGT[rng.below(4)];
                        continue;
                    }
                    uint8_t c = text[p++];
                    if (rng.chance(0.01)) c = ACGT[rng.below(4)];
                    if (rng.chance(0.002)) c = 'N';
                    tmp[i++] = c;
                }
                if (rng.chance(0.5)) {
                    for (uint32_t k = 0; k < read_len; k++) {
                        uint8_t c = tmp[read_len - 1 - k];
                        dst[k] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
                    }
                } else {
                    memcpy(dst, tmp.data(), read_len);
                }
            }
        });
    })
}

}  // extern "C"
