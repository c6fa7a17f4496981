// mtsv-collapse -- merge the result files of several mtsv-binner runs (one per index chunk), as
// src/collapse.rs:543-654 / src/bin/mtsv-collapse.rs:14-89 do: group lines by read id, keep the
// smallest edit per TaxId (mode taxid) or per (TaxId, GI) with the smallest offset as tie-break
// (mode taxid-gi), write one line per read id in ascending read-id order, optional per-TaxId
// report (collapse.rs:717-753).  Host-side text processing: SURVEY 8(f) rank 2, needed to score
// BASELINE config 5 (one index chunk per GPU, reads broadcast).  Inputs are sorted externally in runs of
// 128 MiB (collapse.rs:427-475,665), so result files larger than memory collapse too.
//
// --on-gpu [--device N]: the same output from the device.  The files are mapped and cut into lines, the distinct read IDs
// sorted into a dictionary (collapse_lines.hpp), and the hit parts go, piece by piece through page-locked staging, to
// mtsv_fold_add_text: k_parse.hip turns the text into records in HBM, k_fold.hip merges them, k_fold_report counts the
// report and k_text.hip writes the lines.  Input the device path refuses -- a token outside the canonical grammar, a line
// whose keys do not ascend, taxid-gi mode on tokens without an offset -- goes to the host path below as a whole, before the
// output file is created, so every error text and exit code stays this file's.  Without --on-gpu no device is opened.
//
// --taxonomy <nodes.dmp> with --lca-output and/or --clade-report (only with --on-gpu): what the reads ARE.  mtsv_fold_lca
// (k_lca.hip) takes the fold the -o lines come from and gives a second fold with one record per read -- the lowest common
// ancestor of the read's best taxa (--lca-slack N: of the taxa within N edits of the best; all: of all of them) -- whose
// lines, READ_ID:LCA=EDIT in the order of -o's, are --lca-output, and the reads per clade, --clade-report.  -o and --report
// are what they are without these options.  The host path has no such step: where --on-gpu alone would hand the input to
// it, a run with --taxonomy ends with the reason on stderr, exit code 2 and none of the two files.
//
// --abundance <TSV> [--reassigned <PATH>] (only with --on-gpu): how much of each taxon.  mtsv_fold_abundance (k_abund.hip)
// runs expectation-maximisation over the ambiguous reads of the same fold: a read is shared among its taxa in proportion to the
// taxon's current abundance times --abundance-mismatch Q (default 0.25) to the power of the edits above the read's best, for
// up to --abundance-iters iterations (100) or until the masses move by no more than --abundance-tol reads (0.01);
// --abundance-slack N keeps only the taxa within N edits of the read's best (default all).  --abundance is the TSV of masses and
// counts, --reassigned the lines READ_ID:TAXID=EDIT of the one taxon every read is assigned to, in the order of -o's.  -o and
// --report are unchanged; refused input ends as with --taxonomy.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include <unistd.h>

#include <chrono>

#include "../../include/mtsv_amd.h"
#include "collapse_lines.hpp"

namespace {

[[noreturn]] void die(const std::string& m) {
    fprintf(stderr, "thread 'main' panicked: Problem collapsing files: %s\n", m.c_str());
    exit(101);
}

struct Hit {
    uint32_t tax, gi;
    uint64_t off;
    uint32_t edit;
    bool has_gi, has_off;
};

bool parse_u64(const std::string& s, uint64_t max, uint64_t* out) {
    if (s.empty()) return false;
    uint64_t v = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + (uint64_t)(c - '0');
        if (v > max) return false;
    }
    *out = v;
    return true;
}

// parse_hit_token, collapse.rs:198-255: tax[-gi[-offset]]=edit
Hit parse_token(const std::string& tok) {
    size_t eq = tok.find('=');
    if (eq == std::string::npos || tok.find('=', eq + 1) != std::string::npos) die("InvalidHeader(" + tok + ")");
    std::string left = tok.substr(0, eq);
    uint64_t v;
    Hit h{0, 0, 0, 0, false, false};
    if (!parse_u64(tok.substr(eq + 1), 0xffffffffull, &v)) die("InvalidInteger(" + tok.substr(eq + 1) + ")");
    h.edit = (uint32_t)v;
    std::vector<std::string> parts;
    size_t p = 0;
    for (;;) {
        size_t d = left.find('-', p);
        parts.push_back(left.substr(p, d == std::string::npos ? std::string::npos : d - p));
        if (d == std::string::npos) break;
        p = d + 1;
    }
    if (parts.size() > 3) die("InvalidHeader(" + tok + ")");
    if (!parse_u64(parts[0], 0xffffffffull, &v)) die("InvalidInteger(" + parts[0] + ")");
    h.tax = (uint32_t)v;
    if (parts.size() > 1) {
        if (!parse_u64(parts[1], 0xffffffffull, &v)) die("InvalidInteger(" + parts[1] + ")");
        h.gi = (uint32_t)v;
        h.has_gi = true;
    }
    if (parts.size() > 2) {
        if (!parse_u64(parts[2], ~0ull / 10, &v)) die("InvalidInteger(" + parts[2] + ")");
        h.off = v;
        h.has_off = true;
    }
    return h;
}

struct Stats {
    uint64_t only_hit = 0, only_best = 0, tied_best = 0, not_best = 0;
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

constexpr int kGpuFallBack = -1000;  // run_on_gpu: the input is the host path's

struct LcaOptions {
    std::string taxonomy, lca_output, clade_report;
    uint32_t slack = 0;
    bool on() const { return !taxonomy.empty(); }
};

struct AbundOptions {
    std::string table, reassigned;
    double mismatch = 0.25;
    uint32_t slack = 0xffffffffu, iters = 100;
    uint64_t tol = 42949672;  // floor(0.01 * 2^32)
    bool on() const { return !table.empty(); }
};
constexpr uint32_t kAbundWeights = 64;

bool write_file(const std::string& path, const char* p, uint64_t len) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool wrote = fwrite(p, 1, (size_t)len, f) == len;
    return (fclose(f) == 0) && wrote;
}

// mtsv-collapse --on-gpu.  Returns the exit code, or kGpuFallBack with nothing written.
int run_on_gpu(const std::vector<std::string>& files, const std::string& out_path, const std::string& report, bool by_gi, int device, bool verbose,
               const LcaOptions& lca, const AbundOptions& abund) {
    namespace mc = mtsv_collapse;
    const bool timing = getenv("MTSV_COLLAPSE_TIMING") != nullptr;
    auto fall_back = [&](const std::string& why) {
        if (lca.on() || abund.on()) {  // (the host path has no LCA step and no abundance step)
            fprintf(stderr, "mtsv-collapse: --on-gpu: %s; %s needs the device path\n", why.c_str(), lca.on() ? "--taxonomy" : "--abundance");
            return 2;
        }
        if (verbose) fprintf(stderr, "mtsv-collapse: --on-gpu: %s; the host path takes the input\n", why.c_str());
        return kGpuFallBack;
    };
    auto device_error = [&](const char* what) {
        fprintf(stderr, "mtsv-collapse: --on-gpu: %s: %s\n", what, mtsv_last_error());
        return 2;
    };
    uint64_t piece_bytes = 64ull << 20;
    if (const char* e = getenv("MTSV_COLLAPSE_PIECE_BYTES")) piece_bytes = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
    struct TaxonomyCloser {
        mtsv_taxonomy* tx = nullptr;
        mtsv_fold* per_read = nullptr;  // the fold of the reads' LCA records
        ~TaxonomyCloser() {
            mtsv_fold_free(per_read);
            mtsv_taxonomy_free(tx);
        }
    } tax;
    if (lca.on() && mtsv_taxonomy_load(lca.taxonomy.c_str(), &tax.tx) != MTSV_OK) {
        fprintf(stderr, "mtsv-collapse: --taxonomy: %s\n", mtsv_last_error());
        return 2;
    }
    // ---- lines and dictionary ----
    const double t0 = now_ms();
    std::vector<mc::FileBytes> bytes(files.size());
    std::vector<std::vector<mc::Line>> lines(files.size());
    for (size_t f = 0; f < files.size(); f++) {
        if (!bytes[f].open(files[f])) return fall_back("cannot read " + files[f]);
        std::string bad;
        if (!mc::split_lines(bytes[f].p, bytes[f].n, lines[f], &bad)) return fall_back("a line of " + files[f] + " has no read ID");
        for (const auto& l : lines[f])
            if (l.id_len > (1ull << 20) || memchr(l.id, 0, (size_t)l.id_len)) return fall_back("a read ID of " + files[f] + " holds a NUL or more than 2^20 bytes");
    }
    std::vector<const mc::Line*> dict;
    if (!mc::build_dictionary(lines, dict)) return fall_back("2^32 read IDs or more");
    const uint64_t n_reads = dict.size();
    const double t1 = now_ms();
    // ---- the fold ----
    mtsv_fold* fold = nullptr;
    if (mtsv_fold_create(device, by_gi ? MTSV_GRAIN_TAXID_GI : MTSV_GRAIN_TAXID, &fold) != MTSV_OK) return device_error("no fold on the device");
    struct Closer {
        mtsv_fold* f;
        char* stage = nullptr;
        ~Closer() {
            if (stage) mtsv_host_free(stage);
            mtsv_fold_free(f);
        }
    } hold{fold};
    if (mtsv_fold_reset(fold, n_reads) != MTSV_OK) return device_error("mtsv_fold_reset");
    double stage_ms = 0, add_ms = 0;
    uint64_t stage_cap = 0, n_calls = 0, n_tokens = 0, n_bytes = 0;
    std::vector<const mc::Line*> order;
    std::vector<mc::Piece> pieces;
    std::vector<uint64_t> line_off;
    std::vector<uint32_t> line_read;
    for (size_t f = 0; f < files.size(); f++) {
        const double ta = now_ms();
        mc::cut_pieces(lines[f], piece_bytes, order, pieces);
        stage_ms += now_ms() - ta;
        for (const auto& p : pieces) {
            const double tb = now_ms();
            if (p.bytes > stage_cap || !hold.stage) {
                if (hold.stage) mtsv_host_free(hold.stage);
                // (room for the largest piece of this file: page-locking memory costs by the byte, and files are of a size)
                stage_cap = 4096;
                for (const auto& q : pieces) stage_cap = std::max(stage_cap, q.bytes + q.bytes / 8);
                hold.stage = (char*)mtsv_host_alloc((size_t)stage_cap);
                if (!hold.stage) return device_error("no page-locked staging");
            }
            mc::stage_piece(order, p, hold.stage, line_off, line_read);
            const double tc = now_ms();
            uint64_t tok = 0, rec = 0;
            const int rc = mtsv_fold_add_text(fold, hold.stage, line_off.data(), line_read.data(), line_read.size(), &tok, &rec, nullptr);
            stage_ms += tc - tb;
            add_ms += now_ms() - tc;
            n_calls++;
            n_tokens += tok;
            n_bytes += p.bytes;
            if (rc == MTSV_OK) continue;
            const std::string why = mtsv_last_error();
            if (rc == MTSV_E_FORMAT || rc == MTSV_E_LIMIT || (rc == MTSV_E_ARG && why.find("a key below") != std::string::npos))
                return fall_back(files[f] + ": " + why);
            return device_error("mtsv_fold_add_text");
        }
    }
    // ---- the lines and the report come from the fold ----
    const double t2 = now_ms();
    std::string ids;
    std::vector<uint64_t> id_off(n_reads + 1, 0);
    for (uint64_t r = 0; r < n_reads; r++) {
        ids.append(dict[r]->id, (size_t)dict[r]->id_len);
        id_off[r + 1] = ids.size();
    }
    if (ids.empty()) ids.push_back('\0');  // (a pointer the library accepts)
    char* text = nullptr;
    uint64_t text_len = 0;
    if (mtsv_fold_format_text(fold, ids.data(), id_off.data(), n_reads, &text, &text_len, nullptr) != MTSV_OK) return device_error("mtsv_fold_format_text");
    const double t3 = now_ms();
    char* rep_text = nullptr;
    uint64_t rep_len = 0;
    if (!report.empty()) {
        mtsv_taxon_stats* rows = nullptr;
        uint64_t n_rows = 0, total_reads = 0;
        if (mtsv_fold_taxa_report(fold, &rows, &n_rows, &total_reads, nullptr) != MTSV_OK) {
            mtsv_free(text);
            return device_error("mtsv_fold_taxa_report");
        }
        const int rc = mtsv_format_taxa_report(rows, n_rows, total_reads, &rep_text, &rep_len);
        mtsv_free(rows);
        if (rc != MTSV_OK) {
            mtsv_free(text);
            return device_error("mtsv_format_taxa_report");
        }
    }
    // ---- the reads' LCAs and the clades, from the same fold; both texts are complete before a file is created ----
    char *lca_text = nullptr, *clade_text = nullptr;
    uint64_t lca_len = 0, clade_len = 0;
    struct TextCloser {
        char *&a, *&b;
        ~TextCloser() {
            mtsv_free(a);
            mtsv_free(b);
        }
    } lca_hold{lca_text, clade_text};
    if (lca.on()) {
        auto lca_error = [&](const char* what) {
            mtsv_free(text);
            mtsv_free(rep_text);
            return device_error(what);
        };
        const bool want_lines = !lca.lca_output.empty(), want_clades = !lca.clade_report.empty();
        if (want_lines && mtsv_fold_create(device, MTSV_GRAIN_TAXID, &tax.per_read) != MTSV_OK) return lca_error("no fold for the reads' LCAs");
        mtsv_clade_stats* rows = nullptr;
        uint64_t n_rows = 0, lca_reads = 0;
        if (mtsv_fold_lca(fold, tax.tx, lca.slack, tax.per_read, want_clades ? &rows : nullptr, &n_rows, &lca_reads, nullptr) != MTSV_OK)
            return lca_error("mtsv_fold_lca");
        if (want_clades) {
            const int rc = mtsv_format_clade_report(rows, n_rows, lca_reads, tax.tx, &clade_text, &clade_len);
            mtsv_free(rows);
            if (rc != MTSV_OK) return lca_error("mtsv_format_clade_report");
        }
        if (want_lines && mtsv_fold_format_text(tax.per_read, ids.data(), id_off.data(), n_reads, &lca_text, &lca_len, nullptr) != MTSV_OK)
            return lca_error("mtsv_fold_format_text (LCA lines)");
    }
    // ---- the abundances and the reads' one taxon, from the same fold; both texts are complete before a file is created ----
    char *abund_text = nullptr, *reassigned_text = nullptr;
    uint64_t abund_len = 0, reassigned_len = 0;
    TextCloser abund_hold{abund_text, reassigned_text};
    struct FoldCloser {
        mtsv_fold* f = nullptr;
        ~FoldCloser() { mtsv_fold_free(f); }
    } assigned;
    if (abund.on()) {
        auto abund_error = [&](const char* what) {
            mtsv_free(text);
            mtsv_free(rep_text);
            return device_error(what);
        };
        uint32_t w[kAbundWeights];
        if (mtsv_abundance_weights(abund.mismatch, kAbundWeights, w) != MTSV_OK) return abund_error("mtsv_abundance_weights");
        const bool want_lines = !abund.reassigned.empty();
        if (want_lines && mtsv_fold_create(device, MTSV_GRAIN_TAXID, &assigned.f) != MTSV_OK) return abund_error("no fold for the reads' assignments");
        mtsv_abundance_row* rows = nullptr;
        uint64_t n_rows = 0;
        mtsv_abundance_info info;
        if (mtsv_fold_abundance(fold, w, kAbundWeights, abund.slack, abund.iters, abund.tol, assigned.f, &rows, &n_rows, &info, nullptr) != MTSV_OK)
            return abund_error("mtsv_fold_abundance");
        const int rc = mtsv_format_abundance(rows, n_rows, &info, &abund_text, &abund_len);
        mtsv_free(rows);
        if (rc != MTSV_OK) return abund_error("mtsv_format_abundance");
        if (want_lines && mtsv_fold_format_text(assigned.f, ids.data(), id_off.data(), n_reads, &reassigned_text, &reassigned_len, nullptr) != MTSV_OK)
            return abund_error("mtsv_fold_format_text (reassigned lines)");
        if (verbose)
            fprintf(stderr, "mtsv-collapse: --abundance: %llu reads, %llu entries, %llu taxa, %u iterations, %s\n", (unsigned long long)info.reads,
                    (unsigned long long)info.entries, (unsigned long long)info.taxa, info.iterations, info.converged ? "converged" : "stopped at the cap");
    }
    const double t4 = now_ms();
    FILE* out = fopen(out_path.c_str(), "wb");
    if (!out) {
        fprintf(stderr, "thread 'main' panicked: Unable to create output file.\n");
        mtsv_free(text);
        mtsv_free(rep_text);
        return 101;
    }
    const bool wrote = fwrite(text, 1, (size_t)text_len, out) == text_len;
    mtsv_free(text);
    if (fclose(out) != 0 || !wrote) {
        mtsv_free(rep_text);
        die("write error");
    }
    if (!report.empty()) {
        FILE* r = fopen(report.c_str(), "wb");
        if (!r) {
            fprintf(stderr, "thread 'main' panicked: Unable to write taxa report\n");
            mtsv_free(rep_text);
            return 101;
        }
        fwrite(rep_text, 1, (size_t)rep_len, r);
        fclose(r);
        mtsv_free(rep_text);
    }
    if (lca.on()) {
        const bool ok = (lca.lca_output.empty() || write_file(lca.lca_output, lca_text, lca_len)) &&
                        (lca.clade_report.empty() || write_file(lca.clade_report, clade_text, clade_len));
        if (!ok) {
            if (!lca.lca_output.empty()) remove(lca.lca_output.c_str());
            if (!lca.clade_report.empty()) remove(lca.clade_report.c_str());
            fprintf(stderr, "thread 'main' panicked: Unable to write the LCA output or the clade report\n");
            return 101;
        }
    }
    if (abund.on()) {
        const bool ok = write_file(abund.table, abund_text, abund_len) && (abund.reassigned.empty() || write_file(abund.reassigned, reassigned_text, reassigned_len));
        if (!ok) {
            remove(abund.table.c_str());
            if (!abund.reassigned.empty()) remove(abund.reassigned.c_str());
            fprintf(stderr, "thread 'main' panicked: Unable to write the abundance table or the reassigned lines\n");
            return 101;
        }
    }
    const double t5 = now_ms();
    // MTSV_COLLAPSE_TIMING=1: where the device path spends its time (tools/collapse_ab.py reads this line)
    if (timing)
        fprintf(stderr, "[collapse timing] files %zu reads %llu calls %llu hit_bytes %llu tokens %llu text_bytes %llu; read_split_dictionary %.3f ms, staging %.3f ms, "
                        "add_text %.3f ms, id_table_and_text %.3f ms, report %.3f ms, write %.3f ms\n",
                files.size(), (unsigned long long)n_reads, (unsigned long long)n_calls, (unsigned long long)n_bytes, (unsigned long long)n_tokens,
                (unsigned long long)text_len, t1 - t0, stage_ms, add_ms, t3 - t2, t4 - t3, t5 - t4);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    std::string out_path, mode = "taxid", report;
    std::vector<std::string> files;
    bool on_gpu = false, verbose = false, device_given = false;
    int device = 0;
    LcaOptions lca;
    bool slack_given = false;
    AbundOptions abund;
    const char* abund_given[4] = {nullptr, nullptr, nullptr, nullptr};  // the options that need --abundance, as they were met
    for (int i = 1; i < argc; i++) {
        std::string k = argv[i];
        auto val = [&]() -> std::string {
            if (i + 1 >= argc) {
                fprintf(stderr, "error: The argument '%s' requires a value but none was supplied\n", k.c_str());
                exit(1);
            }
            return argv[++i];
        };
        if (k == "-o" || k == "--output") out_path = val();
        else if (k == "--mode") mode = val();
        else if (k == "-t" || k == "--threads") (void)val();
        else if (k == "--report") report = val();
        else if (k == "-v") verbose = true;
        else if (k == "--on-gpu") on_gpu = true;
        else if (k == "--taxonomy") lca.taxonomy = val();
        else if (k == "--lca-output") lca.lca_output = val();
        else if (k == "--clade-report") lca.clade_report = val();
        else if (k == "--lca-slack") {
            const std::string v = val();
            uint64_t n = 0;
            if (v == "all") n = 0xffffffffull;
            else if (!parse_u64(v, 0xffffffffull, &n)) {
                fprintf(stderr, "error: Invalid value for '--lca-slack <N|all>': %s\n", v.c_str());
                return 1;
            }
            lca.slack = (uint32_t)n;
            slack_given = true;
        }
        else if (k == "--abundance") abund.table = val();
        else if (k == "--reassigned") abund.reassigned = val();
        else if (k == "--abundance-mismatch") {
            const std::string v = val();
            char* end = nullptr;
            abund.mismatch = strtod(v.c_str(), &end);
            if (v.empty() || *end || !(abund.mismatch > 0.0) || !(abund.mismatch <= 1.0)) {
                fprintf(stderr, "error: Invalid value for '--abundance-mismatch <Q>': %s\n", v.c_str());
                return 1;
            }
            abund_given[0] = "--abundance-mismatch <Q>";
        } else if (k == "--abundance-slack") {
            const std::string v = val();
            uint64_t n = 0;
            if (v == "all") n = 0xffffffffull;
            else if (!parse_u64(v, 0xffffffffull, &n)) {
                fprintf(stderr, "error: Invalid value for '--abundance-slack <N|all>': %s\n", v.c_str());
                return 1;
            }
            abund.slack = (uint32_t)n;
            abund_given[1] = "--abundance-slack <N|all>";
        } else if (k == "--abundance-iters") {
            const std::string v = val();
            uint64_t n = 0;
            if (!parse_u64(v, 0xffffffffull, &n)) {
                fprintf(stderr, "error: Invalid value for '--abundance-iters <N>': %s\n", v.c_str());
                return 1;
            }
            abund.iters = (uint32_t)n;
            abund_given[2] = "--abundance-iters <N>";
        } else if (k == "--abundance-tol") {
            const std::string v = val();
            char* end = nullptr;
            const double reads = strtod(v.c_str(), &end);
            if (v.empty() || *end || !(reads >= 0.0) || !(reads < 4294967296.0)) {  // (reads * 2^32 must fit 64 bits)
                fprintf(stderr, "error: Invalid value for '--abundance-tol <READS>': %s\n", v.c_str());
                return 1;
            }
            abund.tol = (uint64_t)(reads * 4294967296.0);  // (the product is exact but for its exponent: the cast is the floor)
            abund_given[3] = "--abundance-tol <READS>";
        } else if (k == "--device") {
            const std::string v = val();
            char* end = nullptr;
            const long d = strtol(v.c_str(), &end, 10);
            if (v.empty() || *end || d < 0 || d > 1 << 20) {
                fprintf(stderr, "error: Invalid value for '--device <N>': %s\n", v.c_str());
                return 1;
            }
            device = (int)d;
            device_given = true;
        } else if (k == "-h" || k == "--help") {
            printf("mtsv-collapse -o <OUTPUT> [--mode taxid|taxid-gi] [--report <TSV>] [-t N] [--on-gpu [--device N] [--taxonomy <nodes.dmp> "
                   "[--lca-output <PATH>] [--clade-report <TSV>] [--lca-slack <N|all>]] [--abundance <TSV> [--abundance-mismatch <Q>] "
                   "[--abundance-slack <N|all>] [--abundance-iters <N>] [--abundance-tol <READS>] [--reassigned <PATH>]]] <FILES>...\n");
            return 0;
        } else if (!k.empty() && k[0] == '-') {
            fprintf(stderr, "error: Found argument '%s' which wasn't expected\n", k.c_str());
            return 1;
        } else
            files.push_back(k);
    }
    if (out_path.empty() || files.empty() || (mode != "taxid" && mode != "taxid-gi")) {
        fprintf(stderr, "error: required: -o <OUTPUT> <FILES>..., --mode taxid|taxid-gi\n");
        return 1;
    }
    if (device_given && !on_gpu) {
        fprintf(stderr, "error: The argument '--device <N>' requires '--on-gpu'\n");
        return 1;
    }
    if (lca.on() && !on_gpu) {
        fprintf(stderr, "error: The argument '--taxonomy <nodes.dmp>' requires '--on-gpu'\n");
        return 1;
    }
    if (lca.on() && lca.lca_output.empty() && lca.clade_report.empty()) {
        fprintf(stderr, "error: The argument '--taxonomy <nodes.dmp>' requires '--lca-output <PATH>' or '--clade-report <TSV>'\n");
        return 1;
    }
    for (const auto& o : {std::make_pair("--lca-output <PATH>", !lca.lca_output.empty()), std::make_pair("--clade-report <TSV>", !lca.clade_report.empty()),
                          std::make_pair("--lca-slack <N|all>", slack_given)})
        if (o.second && !lca.on()) {
            fprintf(stderr, "error: The argument '%s' requires '--taxonomy <nodes.dmp>'\n", o.first);
            return 1;
        }
    if (abund.on() && !on_gpu) {
        fprintf(stderr, "error: The argument '--abundance <TSV>' requires '--on-gpu'\n");
        return 1;
    }
    if (!abund.on()) {
        if (!abund.reassigned.empty()) {
            fprintf(stderr, "error: The argument '--reassigned <PATH>' requires '--abundance <TSV>'\n");
            return 1;
        }
        for (const char* o : abund_given)
            if (o) {
                fprintf(stderr, "error: The argument '%s' requires '--abundance <TSV>'\n", o);
                return 1;
            }
    }
    const bool by_gi = mode == "taxid-gi";
    if (on_gpu) {
        const int rc = run_on_gpu(files, out_path, report, by_gi, device, verbose, lca, abund);
        if (rc != kGpuFallBack) return rc;
    }

    // External sort like collapse.rs:427-475,665: every input is cut into runs of at most `chunk_bytes` of
    // lines (128 MiB there and here; MTSV_COLLAPSE_CHUNK_BYTES for tests), each run is sorted by read id and
    // -- unless it is the last, still in memory -- written to a temporary directory; then one k-way merge over
    // all runs of all files (the reference merges per file first, then across files: same stream) feeds the
    // grouping loop of collapse.rs:543-654.  Memory: one run per input file at a time, one line per run later.
    uint64_t chunk_bytes = 128ull << 20;
    if (const char* e = getenv("MTSV_COLLAPSE_CHUNK_BYTES")) chunk_bytes = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
    struct Rec {
        std::string id, hits;
    };
    struct Run {
        std::vector<Rec> mem;  // in-memory run (sorted), or empty when spilled
        size_t at = 0;
        std::string path;
        std::unique_ptr<std::ifstream> in;
        Rec cur;
        bool next() {  // advance to the next record; false at the end
            if (in) {
                std::string l;
                if (!std::getline(*in, l)) return false;
                const size_t c = l.rfind(':');
                cur.id = l.substr(0, c);
                cur.hits = l.substr(c + 1);
                return true;
            }
            if (at >= mem.size()) return false;
            cur = std::move(mem[at++]);
            return true;
        }
    };
    std::vector<std::unique_ptr<Run>> runs;
    std::string tmp_dir;
    auto spill = [&](std::vector<Rec>& recs) {
        if (tmp_dir.empty()) {
            const char* base = getenv("TMPDIR");
            std::string t = std::string(base && *base ? base : "/tmp") + "/mtsv-collapse-XXXXXX";
            std::vector<char> buf(t.begin(), t.end());
            buf.push_back('\0');
            if (!mkdtemp(buf.data())) die("cannot create a temporary directory under " + t);
            tmp_dir = buf.data();
        }
        auto r = std::make_unique<Run>();
        r->path = tmp_dir + "/run-" + std::to_string(runs.size()) + ".txt";
        FILE* f = fopen(r->path.c_str(), "wb");
        if (!f) die("cannot write " + r->path);
        for (auto& rec : recs) {
            if (fwrite(rec.id.data(), 1, rec.id.size(), f) != rec.id.size() || fputc(':', f) == EOF ||
                fwrite(rec.hits.data(), 1, rec.hits.size(), f) != rec.hits.size() || fputc('\n', f) == EOF)
                die("write error in " + r->path);
        }
        if (fclose(f) != 0) die("write error in " + r->path);
        recs.clear();
        recs.shrink_to_fit();
        runs.push_back(std::move(r));
    };
    auto by_id = [](const Rec& a, const Rec& b) { return a.id < b.id; };
    for (size_t f = 0; f < files.size(); f++) {
        std::ifstream in(files[f], std::ios::binary);
        if (!in) die("cannot open " + files[f]);
        std::vector<Rec> recs;
        uint64_t bytes = 0;
        std::string l;
        while (std::getline(in, l)) {
            while (!l.empty() && (l.back() == '\r' || l.back() == '\n')) l.pop_back();
            if (l.find_first_not_of(" \t") == std::string::npos) continue;
            size_t c = l.rfind(':');  // rsplitn(2, ':'), collapse.rs:180-191
            if (c == std::string::npos || c == 0) die("InvalidHeader(" + l + ")");
            bytes += l.size() + 1;
            recs.push_back(Rec{l.substr(0, c), l.substr(c + 1)});
            if (bytes >= chunk_bytes) {
                std::stable_sort(recs.begin(), recs.end(), by_id);
                spill(recs);
                bytes = 0;
            }
        }
        if (!recs.empty()) {
            std::stable_sort(recs.begin(), recs.end(), by_id);
            auto r = std::make_unique<Run>();
            r->mem = std::move(recs);
            runs.push_back(std::move(r));
        }
    }
    for (auto& r : runs)
        if (!r->path.empty()) {
            r->in = std::make_unique<std::ifstream>(r->path, std::ios::binary);
            if (!*r->in) die("cannot reopen " + r->path);
        }
    // min-heap over the runs' current records: (read id, run index) like collapse.rs:553-566
    auto later = [&](size_t a, size_t b) {
        const int c = runs[a]->cur.id.compare(runs[b]->cur.id);
        return c != 0 ? c > 0 : a > b;
    };
    std::vector<size_t> heap;
    for (size_t k = 0; k < runs.size(); k++)
        if (runs[k]->next()) heap.push_back(k);
    std::make_heap(heap.begin(), heap.end(), later);

    FILE* out = fopen(out_path.c_str(), "wb");
    if (!out) {
        fprintf(stderr, "thread 'main' panicked: Unable to create output file.\n");
        return 101;
    }
    std::map<uint32_t, Stats> stats;
    uint64_t total_reads = 0;
    int offset_format = -1;  // unknown / 0 / 1
    std::string text, cur_id;
    char num[96];
    while (!heap.empty()) {
        cur_id = runs[heap.front()]->cur.id;
        std::map<uint32_t, uint32_t> tax_hits;                                      // taxid -> min edit
        std::map<std::pair<uint32_t, uint32_t>, std::pair<uint32_t, uint64_t>> gi_hits;  // (taxid, gi) -> (edit, offset)
        while (!heap.empty() && runs[heap.front()]->cur.id == cur_id) {
            std::pop_heap(heap.begin(), heap.end(), later);
            const size_t k = heap.back();
            const std::string hs = std::move(runs[k]->cur.hits);
            if (runs[k]->next()) std::push_heap(heap.begin(), heap.end(), later);
            else heap.pop_back();
            size_t p = 0;
            while (!hs.empty()) {
                size_t c = hs.find(',', p);
                Hit h = parse_token(hs.substr(p, c == std::string::npos ? std::string::npos : c - p));
                if (!by_gi) {
                    auto it = tax_hits.find(h.tax);
                    if (it == tax_hits.end()) tax_hits[h.tax] = h.edit;
                    else if (h.edit < it->second) it->second = h.edit;
                } else {
                    if (!h.has_gi) die("InvalidHeader(Missing GI for taxid-gi collapse)");
                    if (offset_format >= 0 && (offset_format == 1) != h.has_off) die("InvalidHeader(Mixed offset formats in collapse input)");
                    offset_format = h.has_off ? 1 : 0;
                    auto key = std::make_pair(h.tax, h.gi);
                    auto it = gi_hits.find(key);
                    if (it == gi_hits.end()) gi_hits[key] = {h.edit, h.off};
                    else if (h.edit < it->second.first || (h.edit == it->second.first && h.off < it->second.second)) it->second = {h.edit, h.off};
                }
                if (c == std::string::npos) break;
                p = c + 1;
            }
        }
        // per-taxid summary + stats (collapse.rs:94-147)
        std::map<uint32_t, uint32_t> summary;
        if (!by_gi) summary = tax_hits;
        else
            for (auto& kv : gi_hits) {
                auto it = summary.find(kv.first.first);
                if (it == summary.end()) summary[kv.first.first] = kv.second.first;
                else if (kv.second.first < it->second) it->second = kv.second.first;
            }
        if (!summary.empty()) {
            uint32_t mn = 0xffffffffu;
            for (auto& kv : summary) mn = std::min(mn, kv.second);
            size_t best = 0;
            for (auto& kv : summary) best += kv.second == mn;
            total_reads++;
            for (auto& kv : summary) {
                Stats& s = stats[kv.first];
                if (summary.size() == 1) s.only_hit++;
                else if (kv.second == mn) (best == 1 ? s.only_best : s.tied_best)++;
                else s.not_best++;
            }
        }
        // write (collapse.rs:269-337)
        text.clear();
        bool any = false;
        if (!by_gi) {
            for (auto& kv : tax_hits) {
                snprintf(num, sizeof num, "%s%u=%u", any ? "," : "", kv.first, kv.second);
                text += num;
                any = true;
            }
        } else {
            for (auto& kv : gi_hits) {
                if (offset_format == 1)
                    snprintf(num, sizeof num, "%s%u-%u-%llu=%u", any ? "," : "", kv.first.first, kv.first.second,
                             (unsigned long long)kv.second.second, kv.second.first);
                else
                    snprintf(num, sizeof num, "%s%u-%u=%u", any ? "," : "", kv.first.first, kv.first.second, kv.second.first);
                text += num;
                any = true;
            }
        }
        if (any) fprintf(out, "%s:%s\n", cur_id.c_str(), text.c_str());
    }
    for (auto& r : runs)
        if (!r->path.empty()) {
            r->in.reset();
            remove(r->path.c_str());
        }
    if (!tmp_dir.empty()) rmdir(tmp_dir.c_str());
    if (fclose(out) != 0) die("write error");
    if (!report.empty()) {
        FILE* r = fopen(report.c_str(), "wb");
        if (!r) {
            fprintf(stderr, "thread 'main' panicked: Unable to write taxa report\n");
            return 101;
        }
        fprintf(r, "taxid\tonly_hit\tonly_hit_pct\tonly_best\tonly_best_pct\ttied_best\ttied_best_pct\tnot_best\tnot_best_pct\ttotal_reads\ttotal_pct\n");
        double denom = (double)std::max<uint64_t>(total_reads, 1);
        for (auto& kv : stats) {
            const Stats& s = kv.second;
            uint64_t tot = s.only_hit + s.only_best + s.tied_best + s.not_best;
            fprintf(r, "%u\t%llu\t%.2f\t%llu\t%.2f\t%llu\t%.2f\t%llu\t%.2f\t%llu\t%.2f\n", kv.first, (unsigned long long)s.only_hit,
                    s.only_hit / denom * 100.0, (unsigned long long)s.only_best, s.only_best / denom * 100.0,
                    (unsigned long long)s.tied_best, s.tied_best / denom * 100.0, (unsigned long long)s.not_best,
                    s.not_best / denom * 100.0, (unsigned long long)tot, tot / denom * 100.0);
        }
        fclose(r);
    }
    return 0;
}
