// mtsv-binner -- drop-in command line of the reference binary (src/bin/mtsv-binner.rs) over
// libmtsv_amd: same flags and defaults (:26-113), same validation (:140-262), same exit codes
// (0 ok, 2 query error, 3 no results path, 4 resume error, 11 write error, 12 read error;
// invalid numbers abort like the reference's panics, exit 101), same results grammar
// (src/binner.rs:310-379), same resume rule (:347-411).  Extras: --device / --devices, --batch-reads,
// --parse-only (ingest check: prints record / base counts and checksums, needs no index or GPU), --report, and
// --matched / --unmatched: the reads of the run split by "the read got a hit", what the reference's mtsv-partition
// (src/bin/mtsv-partition.rs) makes of the results file and a second pass over the reads -- here from one flag bit per
// read that the device sets (k_match.hip), with no results file at all when --results is left out (read depletion).
// A read counts by itself there: mtsv-partition keys reads by their ID text, so two records with one ID share a fate.
// --filter-index F1[,F2,..]: reads that get a hit in any of these indexes are dropped on the device and the rest are binned
// against --index, in one process: the filters' workspaces run flags-only, and the unmatched reads of each stage are handed
// to the next workspace in HBM (mtsv_batch_take_reads) -- what `--unmatched tmp.fq` and a second run do through a file.
// The reads of a batch are processed on the GPU; result lines are written in input order (the
// reference's order is unspecified: vendor/cue/src/lib.rs:67-74).
//
// Several GPUs of one node:
//   --devices 0,1,..  with one --index: the index is loaded once and made resident on every listed device;
//                     worker threads with a workspace each (three per entry, MTSV_CLI_WORKERS) pull groups of read
//                     batches (README.md:69-73 workflow)
//   --index a,b,..    the chunks of a database cut by mtsv-chunk, chunk k on the k-th listed device (round
//                     robin): every chunk sees every batch and the hits are merged per read, so the one results
//                     file equals what mtsv-collapse makes of the per-chunk files (README.md:189,
//                     collapse.rs:597-625: smallest edit per read and TaxId)
//   --merge-on-gpu    with --index a,b,.. and ONE device: every chunk resident there, and a call's hits merged per read in
//                     HBM (mtsv_batch_copy_reads, mtsv_batch_merge_runs) -- the reads go up once per call, and --report,
//                     --matched / --unmatched work on the merged hits as they do for one index
//   --fold-on-gpu     with --index a,b,.. and ONE device: ONE chunk resident at a time -- a database whose chunks do not fit
//                     the device together.  The reads are taken in super-batches (--fold-reads N); per super-batch every
//                     chunk in turn is loaded, made resident, run against the reads and freed, and what outlives it is an
//                     accumulator of collapsed assignment records in HBM (mtsv_fold_add_run); results, --report and
//                     --matched / --unmatched come from the accumulated records, byte for byte what --merge-on-gpu writes
//   --text-on-gpu     with --fold-on-gpu: a piece's result lines are written on the device from the accumulated records
//   --fold-prefetch   with --fold-on-gpu: the next chunk's file is read by a loader thread while the resident chunk runs
//                     (mtsv_fold_format_text, k_text.hip) -- the read IDs go up and the text comes down, where otherwise the
//                     records come down and a host thread formats them; the results file is the same byte for byte
//   --dedup           with --fold-on-gpu: identical reads of a piece are binned once (mtsv_batch_take_unique, k_dedup.hip) and
//                     the records of the one read that ran are fanned out to its copies before anything is derived from them
//                     (mtsv_fold_expand): every output file is the same byte for byte
#include <cstddef>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/mtsv_amd.h"
#include "fastx_ingest.hpp"

namespace {

bool g_verbose = false;
void logmsg(const char* level, const std::string& msg) {
    if (!g_verbose && !strcmp(level, "DEBUG")) return;
    char ts[32];
    time_t t = time(nullptr);
    strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S", localtime(&t));
    printf("[%s %s mtsv_binner] %s\n", level, ts, msg.c_str());  // util.rs:10-24: stdout
    fflush(stdout);
}
[[noreturn]] void panic(const std::string& msg) {  // the reference's expect()/panic!() paths
    fprintf(stderr, "thread 'main' panicked: %s\n", msg.c_str());
    exit(101);
}

using mtsv_ingest::FastxReader;  // the serial reader (fastx_ingest.hpp)
using mtsv_ingest::Record;

// resume_offset_from_results (mtsv-binner.rs:366-396): index of the last input record whose id
// appears in the results file, plus one
int resume_offset(const std::string& results, const std::string& input, bool fastq, uint64_t* off) {
    FILE* f = fopen(results.c_str(), "rb");
    if (!f) return -1;
    std::unordered_set<std::string> ids;
    std::string line;
    char buf[1 << 16];
    auto flush_line = [&](std::string& l) -> bool {
        size_t a = l.find_first_not_of(" \t\r\n");
        if (a != std::string::npos) {
            size_t c = l.rfind(':');
            if (c == std::string::npos || c == 0) return false;  // "Missing read id"
            ids.insert(l.substr(0, c));
        }
        l.clear();
        return true;
    };
    while (fgets(buf, sizeof buf, f)) {
        line += buf;
        if (!line.empty() && line.back() == '\n') {
            line.pop_back();
            if (!flush_line(line)) {
                fclose(f);
                return -1;
            }
        }
    }
    if (!line.empty() && !flush_line(line)) {
        fclose(f);
        return -1;
    }
    fclose(f);
    FastxReader rd;
    rd.fastq = fastq;
    if (!rd.in.open(input)) return -1;
    Record r;
    uint64_t idx = 0, last = 0;
    bool any = false;
    while (rd.next(r)) {
        if (ids.count(r.id)) {
            last = idx;
            any = true;
        }
        idx++;
    }
    if (rd.error) return -1;
    *off = any ? last + 1 : 0;
    return 0;
}

struct Args {
    std::string fasta, fastq, index, results, report, matched, unmatched, filter_index, output_format = "default";
    std::string threads = "4", edit = "0.13", seed_size = "18", seed_interval = "15", min_seed = "0.015",
                max_hits = "2000", tune_max_hits = "200", max_assign, max_cand, read_offset = "0";
    bool verbose = false, force = false, parse_only = false, merge_gpu = false, fold_gpu = false, text_gpu = false, fold_prefetch = false, dedup = false;
    uint64_t fold_reads = 16ull << 20;  // --fold-reads: reads per super-batch of --fold-on-gpu (every chunk is loaded once per super-batch)
    std::vector<int> devices{0};
    uint64_t batch_reads = 1u << 17;  // parser blocks of ~40 MB; the GPU workers take up to 1 Mi reads of them per library call. End to end on 32 M reads: 64 Ki .., 128 Ki 70 M reads/s, 256 Ki 54, 512 Ki 37
};

[[noreturn]] void usage_error(const std::string& m) {
    fprintf(stderr, "error: %s\n\nUSAGE:\n    mtsv-binner [FLAGS] [OPTIONS] --index <INDEX> <--fasta <FASTA>|--fastq <FASTQ>>\n", m.c_str());
    exit(1);  // clap usage errors
}

uint64_t parse_usize(const std::string& s, const char* what) {
    if (s.empty()) panic(what);
    char* e = nullptr;
    errno = 0;
    if (s[0] == '-') panic(what);
    unsigned long long v = strtoull(s.c_str(), &e, 10);
    if (*e || errno) panic(what);
    return v;
}
double parse_f64(const std::string& s, const char* what) {
    char* e = nullptr;
    if (s.empty()) panic(what);
    double v = strtod(s.c_str(), &e);
    if (*e) panic(what);
    return v;
}

}  // namespace

// MTSV_CLI_MARKS=1: the set-up phases on stderr as they end, in ms since the process began
static void setup_mark(const char* what) {
    static const bool on = getenv("MTSV_CLI_MARKS") != nullptr;
    static struct timespec t0 = [] {
        struct timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return t;
    }();
    if (!on) return;
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    fprintf(stderr, "[cli set-up] %9.3f ms  %s\n", ((t.tv_sec - t0.tv_sec) + (t.tv_nsec - t0.tv_nsec) * 1e-9) * 1e3, what);
}

int main(int argc, char** argv) {
    setup_mark("main");
    Args a;
    for (int i = 1; i < argc; i++) {
        std::string k = argv[i];
        auto val = [&]() -> std::string {
            size_t eq = k.find('=');
            if (k.rfind("--", 0) == 0 && eq != std::string::npos) {
                std::string v = k.substr(eq + 1);
                k = k.substr(0, eq);
                return v;
            }
            if (i + 1 >= argc) usage_error("The argument '" + k + "' requires a value but none was supplied");
            return argv[++i];
        };
        std::string key = k.substr(0, k.find('='));
        if (key == "--fasta") a.fasta = val();
        else if (key == "--fastq") a.fastq = val();
        else if (key == "-i" || key == "--index") a.index = val();
        else if (key == "-m" || key == "--results") a.results = val();
        else if (key == "-t" || key == "--threads") a.threads = val();
        else if (key == "-e" || key == "--edit-rate") a.edit = val();
        else if (key == "--seed-size") a.seed_size = val();
        else if (key == "--seed-interval") a.seed_interval = val();
        else if (key == "--min-seed") a.min_seed = val();
        else if (key == "--max-hits") a.max_hits = val();
        else if (key == "--tune-max-hits") a.tune_max_hits = val();
        else if (key == "--max-assignments") a.max_assign = val();
        else if (key == "--max-candidates") a.max_cand = val();
        else if (key == "--read-offset") a.read_offset = val();
        else if (key == "--output-format") a.output_format = val();
        else if (key == "--force-overwrite") a.force = true;
        else if (key == "-v") a.verbose = true;
        else if (key == "--device" || key == "--devices") {
            a.devices.clear();
            const std::string v = val();
            size_t at = 0;
            while (at <= v.size()) {
                size_t c = v.find(',', at);
                if (c == std::string::npos) c = v.size();
                const std::string tok = v.substr(at, c - at);
                char* e = nullptr;
                const long d = strtol(tok.c_str(), &e, 10);
                if (tok.empty() || *e || d < 0 || d > 1023) usage_error("Invalid value for '" + key + "': a comma-separated list of GPU ordinals is expected");
                a.devices.push_back((int)d);
                at = c + 1;
            }
        } else if (key == "--batch-reads") {
            const std::string v = val();
            char* e = nullptr;
            errno = 0;
            const unsigned long long n = strtoull(v.c_str(), &e, 10);
            if (v.empty() || v[0] == '-' || *e || errno || n < 1 || n > 0x7fffffffull)
                usage_error("Invalid value for '--batch-reads <N>': a number of reads between 1 and 2147483647 is expected");
            a.batch_reads = n;
        }
        else if (key == "--report") a.report = val();
        else if (key == "--matched") a.matched = val();
        else if (key == "--unmatched") a.unmatched = val();
        else if (key == "--filter-index") a.filter_index = val();
        else if (key == "--parse-only") a.parse_only = true;
        else if (key == "--merge-on-gpu") a.merge_gpu = true;
        else if (key == "--fold-on-gpu") a.fold_gpu = true;
        else if (key == "--text-on-gpu") a.text_gpu = true;
        else if (key == "--fold-prefetch") a.fold_prefetch = true;
        else if (key == "--dedup") a.dedup = true;
        else if (key == "--fold-reads") {
            const std::string v = val();
            char* e = nullptr;
            errno = 0;
            const unsigned long long n = strtoull(v.c_str(), &e, 10);
            if (v.empty() || v[0] == '-' || *e || errno || n < 1 || n > 0xffffffffull)
                usage_error("Invalid value for '--fold-reads <N>': a number of reads between 1 and 4294967295 is expected");
            a.fold_reads = n;
        }
        else if (key == "-h" || key == "--help") {
            printf("mtsv-binner (MI355X) -- flags as the reference: --fasta|--fastq, -i/--index, -m/--results, -t/--threads,\n"
                   "-e/--edit-rate, --seed-size, --seed-interval, --min-seed, --max-hits, --tune-max-hits, --max-assignments,\n"
                   "--max-candidates, --read-offset, --output-format default|long, --force-overwrite, -v;\n"
                   "extras: --devices 0,1,.. (index replicated, reads shared out), --index a,b,.. (database chunks, one per GPU, hits merged),\n"
                   "--batch-reads N, --parse-only,\n"
                   "--report TSV (per-TaxID read counts of the reads processed by this run, as mtsv-collapse --report writes them: with\n"
                   "--read-offset or a resumed run, the reads binned now; counted on the GPU; not with a list of index chunks),\n"
                   "--matched PATH, --unmatched PATH (either or both: every read processed by this run is written, in input order, to\n"
                   "--matched when it got a hit and to --unmatched when it did not, as mtsv-partition would from the results file; the\n"
                   "decision is one bit per read set on the GPU.  Without -m/--results no results file is written and the hits are not\n"
                   "even gathered: read depletion.  Reads skipped by --read-offset go to neither file; a run that would resume an\n"
                   "existing results file is refused; not with a list of index chunks.  Every read counts by itself: mtsv-partition\n"
                   "keys reads by their ID, so there records that share an ID share a fate),\n"
                   "--filter-index F1[,F2,..] (reads that get a hit in any of these indexes, under the run's own parameters, are dropped\n"
                   "and the rest are binned against --index: every filter index is made resident on each device beside the database --\n"
                   "they share its HBM, and the k-mer table of an index may come out narrower for it -- and the surviving reads go from\n"
                   "stage to stage on the GPU, with no intermediate file.  Not with --matched / --unmatched, --parse-only or a list of\n"
                   "index chunks),\n"
                   "--merge-on-gpu (with --index a,b,.. of two or more chunks and one --devices entry: every chunk is made resident on\n"
                   "that device, a call's reads go up once and are copied from chunk to chunk on the GPU, and the chunks' hits are merged\n"
                   "per read on the GPU; the results file is the same, and --report and --matched / --unmatched are accepted: they are\n"
                   "counted from the merged hits.  Each worker holds a workspace per chunk and one more.  Not with --filter-index),\n"
                   "--fold-on-gpu (with --index a,b,.. of two or more chunks and one --devices entry, for a database whose chunks do not\n"
                   "fit the device together: one chunk is resident at a time.  The reads are taken in super-batches of at most\n"
                   "--fold-reads N reads (default 16777216); per super-batch every chunk in turn is loaded, made resident, run and freed,\n"
                   "and its collapsed assignments are folded into an accumulator of records on the GPU; the results file, --report and\n"
                   "--matched / --unmatched are the same as with --merge-on-gpu.  Not with --merge-on-gpu, --filter-index or\n"
                   "--parse-only; a run that would resume an existing results file is refused),\n"
                   "--text-on-gpu (only with --fold-on-gpu: the result lines are written on the GPU from the accumulated records, and the\n"
                   "text is what comes to the host; the results file is the same),\n"
                   "--fold-prefetch (only with --fold-on-gpu: a loader thread reads chunk c + 1 from its file while chunk c is made\n"
                   "resident, run and folded, and the chunks are packed into the device layout on the GPU; still one chunk resident\n"
                   "at a time, at most two in host memory; the files are the same),\n"
                   "--dedup (only with --fold-on-gpu: reads of a batch that are identical base for base after normalisation are binned\n"
                   "once, on the GPU, and the records of the one that ran are copied to the others on the GPU before results, --report\n"
                   "and --matched / --unmatched are derived; every read keeps its own ID and every file is the same)\n");
            return 0;
        } else if (key == "-V" || key == "--version") {
            printf("mtsv 2.1.0 (%s)\n", mtsv_version());
            return 0;
        } else
            usage_error("Found argument '" + k + "' which wasn't expected, or isn't valid in this context");
    }
    if (a.fasta.empty() == a.fastq.empty())
        usage_error(a.fasta.empty() ? "The following required arguments were not provided: --fasta <FASTA> | --fastq <FASTQ>"
                                    : "The argument '--fasta <FASTA>' cannot be used with '--fastq <FASTQ>'");
    if (a.index.empty() && !a.parse_only) usage_error("The following required arguments were not provided: --index <INDEX>");
    if (a.text_gpu) {
        // (decided here, before any file or device is touched)
        if (a.merge_gpu && !a.fold_gpu) usage_error("The argument '--text-on-gpu' cannot be used with '--merge-on-gpu': it writes the lines of '--fold-on-gpu'");
        if (!a.fold_gpu) usage_error("The argument '--text-on-gpu' requires '--fold-on-gpu'");
    }
    if (a.fold_prefetch && !a.fold_gpu) usage_error("The argument '--fold-prefetch' requires '--fold-on-gpu'");  // (likewise)
    if (a.dedup && !a.fold_gpu) usage_error("The argument '--dedup' requires '--fold-on-gpu'");                  // (likewise)
    if (a.merge_gpu) {
        // (decided here, before any file or device is touched)
        size_t n_chunks = 0;
        for (size_t at = 0; at <= a.index.size();) {
            size_t c = a.index.find(',', at);
            if (c == std::string::npos) c = a.index.size();
            n_chunks += c > at;
            at = c + 1;
        }
        if (n_chunks < 2) {
            fprintf(stderr, "error: '--merge-on-gpu' needs a list of two or more index chunks ('--index a,b,..')\n");
            return 1;
        }
        if (a.devices.size() != 1) {
            fprintf(stderr, "error: '--merge-on-gpu' needs exactly one '--devices' entry: every chunk is made resident on that device\n");
            return 1;
        }
        if (a.parse_only) usage_error("The argument '--parse-only' cannot be used with '--merge-on-gpu'");
    }
    if (a.fold_gpu) {
        // (decided here, before any file or device is touched)
        if (a.merge_gpu) usage_error("The argument '--merge-on-gpu' cannot be used with '--fold-on-gpu'");
        if (!a.filter_index.empty()) usage_error("The argument '--filter-index <INDEX>' cannot be used with '--fold-on-gpu'");
        size_t n_chunks = 0;
        for (size_t at = 0; at <= a.index.size();) {
            size_t c = a.index.find(',', at);
            if (c == std::string::npos) c = a.index.size();
            n_chunks += c > at;
            at = c + 1;
        }
        if (n_chunks < 2) {
            fprintf(stderr, "error: '--fold-on-gpu' needs a list of two or more index chunks ('--index a,b,..')\n");
            return 1;
        }
        if (a.devices.size() != 1) {
            fprintf(stderr, "error: '--fold-on-gpu' needs exactly one '--devices' entry: the chunks take turns on that device\n");
            return 1;
        }
        if (a.parse_only) usage_error("The argument '--parse-only' cannot be used with '--fold-on-gpu'");
    }
    const bool folded = a.fold_gpu;
    const bool merged = a.merge_gpu;
    if (!merged && !folded && !a.report.empty() && a.index.find(',') != std::string::npos) {
        // a read's taxa come from several chunks there and per-chunk counters do not add up
        fprintf(stderr, "error: '--report <TSV>' cannot be used with a list of index chunks ('--index a,b,..'): run mtsv-collapse --report on the results file instead, or give '--merge-on-gpu' (one device)\n");
        return 1;
    }
    const bool partition = !a.matched.empty() || !a.unmatched.empty();
    if (partition && a.parse_only) usage_error("The argument '--parse-only' cannot be used with '--matched <PATH>' / '--unmatched <PATH>'");
    if (!merged && !folded && partition && a.index.find(',') != std::string::npos) {
        // (the flags of the chunks would have to be OR-ed per read)
        fprintf(stderr, "error: '--matched <PATH>' / '--unmatched <PATH>' cannot be used with a list of index chunks ('--index a,b,..'): run mtsv-partition on the results file instead, or give '--merge-on-gpu' (one device)\n");
        return 1;
    }
    const bool filtered = !a.filter_index.empty();
    if (filtered && partition) usage_error("The argument '--filter-index <INDEX>' cannot be used with '--matched <PATH>' / '--unmatched <PATH>'");
    if (filtered && a.parse_only) usage_error("The argument '--parse-only' cannot be used with '--filter-index <INDEX>'");
    if (filtered && a.index.find(',') != std::string::npos) {
        // (every chunk would need the survivors, and its hits merged per read)
        fprintf(stderr, "error: '--filter-index <INDEX>' cannot be used with a list of index chunks ('--index a,b,..'): filter first with '--unmatched <PATH>', then bin the chunks\n");
        return 1;
    }
    if (!merged && !folded && partition && !a.report.empty() && a.results.empty())
        usage_error("The argument '--report <TSV>' requires '-m/--results <RESULTS>': the report is counted from gathered hits, and '--matched' / '--unmatched' without a results file gather none");
    if (a.output_format != "default" && a.output_format != "long")
        usage_error("'" + a.output_format + "' isn't a valid value for '--output-format <OUTPUT_FORMAT>'");
    g_verbose = a.verbose;

    const bool fastq = a.fasta.empty();
    const std::string input = fastq ? a.fastq : a.fasta;
    const uint64_t t_flag = parse_usize(a.threads, "Invalid number entered for number of threads!");
    // -t sized the reference's worker pool; here it sizes the host helper threads (parse, format)
    unsigned host_threads = (unsigned)std::min<uint64_t>(std::max<uint64_t>(t_flag, 8), std::max(1u, std::thread::hardware_concurrency()));
    if (const char* e = getenv("MTSV_HOST_THREADS")) host_threads = (unsigned)std::max(1, atoi(e));
    mtsv_params p;
    mtsv_params_default(&p);
    p.edit_rate = parse_f64(a.edit, "Invalid edit proportion entered!");
    logmsg("INFO", "Max Edit Tolerance Proportion: " + a.edit);
    if (p.edit_rate < 0.0 || p.edit_rate > 1.0) panic("Edit tolerance proportion must be between 0 and 1, inclusive");
    uint64_t seed_size = parse_usize(a.seed_size, "Invalid seed size entered!");
    if (seed_size < 16) logmsg("WARN", "Seed size may be small enough that it causes performance issues.");
    else if (seed_size > 24) logmsg("WARN", "Seed size may be large enough that significant results are ignored.");
    uint64_t seed_gap = parse_usize(a.seed_interval, "Invalid seed interval entered!");
    if (seed_gap < 2) logmsg("WARN", "Seed interval may be small enough that it causes performance issues.");
    else if (seed_gap > 10) logmsg("WARN", "Seed interval may be large enough that significant results are ignored.");
    p.min_seed = parse_f64(a.min_seed, "Invalid min seeds entered!");
    if (p.min_seed <= 0.0 || p.min_seed > 1.0) panic("Min seed percent must be between 0 and 1");
    p.max_hits = parse_usize(a.max_hits, "Invalid cutoff for max hits!");
    p.tune_max_hits = parse_usize(a.tune_max_hits, "Invalid cutoff for max hits!");
    p.max_assignments = a.max_assign.empty() ? -1 : (int64_t)parse_usize(a.max_assign, "Invalid number entered for max assignments!");
    p.max_candidates = a.max_cand.empty() ? -1 : (int64_t)parse_usize(a.max_cand, "Invalid number entered for max candidates!");
    uint64_t read_offset = parse_usize(a.read_offset, "Invalid read offset entered!");
    if (seed_size == 0 || seed_size > 0xffffffffull || seed_gap == 0 || seed_gap > 0xffffffffull)
        panic("seed size / interval out of range");  // the reference panics on a zero step (itertools)
    p.seed_size = (uint32_t)seed_size;
    p.seed_interval = (uint32_t)seed_gap;
    const bool long_fmt = a.output_format == "long";

    const bool have_results = !a.results.empty();
    if (a.results.empty() && !a.parse_only && !partition) {
        logmsg("ERROR", "No results path provided!");
        return 3;
    }
    FILE* probe = have_results ? fopen(a.results.c_str(), "rb") : nullptr;
    const bool exists = probe != nullptr;
    if (probe) fclose(probe);
    const bool append = !a.force && exists;
    uint64_t resume = 0;
    if (a.force) {
        logmsg("INFO", "Forcing overwrite of " + a.results);
    } else if (exists && partition) {
        // a resumed run sees only the reads after the last one in the results file: the partition files would be incomplete
        fprintf(stderr, "error: results file %s exists and the run would resume it; '--matched' / '--unmatched' need the whole input: give --force-overwrite or another results path\n", a.results.c_str());
        return 1;
    } else if (exists && folded) {
        // (the accumulators hold a super-batch of the whole input's numbering; a resumed run is not what this path is for)
        fprintf(stderr, "error: results file %s exists and the run would resume it; '--fold-on-gpu' does not resume: give --force-overwrite or another results path\n", a.results.c_str());
        return 1;
    } else if (exists && !a.parse_only) {
        logmsg("INFO", "Existing results detected at " + a.results + "; resuming previous run.");
        if (resume_offset(a.results, input, fastq, &resume) != 0) {
            logmsg("ERROR", "Error computing resume offset");
            return 4;
        }
        logmsg("INFO", "Resuming after read offset " + std::to_string(resume) + " from " + a.results);
    }
    read_offset += resume;

    // get_fastx_and_write_matching_bin_ids (binner.rs:149-217)
    // Producer: block-parallel ingest for plain files (fastx_ingest.hpp), the serial reader for gzip
    // input and from the first irregular block on.  `emit` gets records in input order.
    using mtsv_ingest::ReadBlock;
    mtsv_ingest::keep_records() = partition;  // descriptions and qualities: only when records are written out again
    FastxReader rd;
    rd.fastq = fastq;
    if (!rd.in.open(input)) {
        logmsg("ERROR", "Error running query: cannot open " + input);
        return 2;
    }
    // batches are recycled (writer -> producer) so that steady state touches no fresh pages
    struct BlockPool {
        std::mutex mu;
        std::vector<std::unique_ptr<ReadBlock>> free;
        std::unique_ptr<ReadBlock> get() {
            std::lock_guard<std::mutex> lk(mu);
            if (free.empty()) return std::make_unique<ReadBlock>();
            auto b = std::move(free.back());
            free.pop_back();
            b->clear();
            return b;
        }
        size_t keep = 8;
        void put(std::unique_ptr<ReadBlock> b) {
            std::lock_guard<std::mutex> lk(mu);
            if (free.size() < keep) free.push_back(std::move(b));
        }
        // a stock of blocks whose (page-locked) base buffers exist before the first query: creating one costs
        // milliseconds per block, which the first second of a run would otherwise spend in its parser threads
        void stock(size_t n, uint64_t base_bytes) {
            keep = std::max(keep, n);
            std::vector<std::thread> th;
            std::vector<std::unique_ptr<ReadBlock>> made(n);
            for (size_t k = 0; k < n; k++)
                th.emplace_back([&made, k, base_bytes] {
                    made[k] = std::make_unique<ReadBlock>();
                    made[k]->bases.reserve(base_bytes);
                });
            for (auto& t : th) t.join();
            std::lock_guard<std::mutex> lk(mu);
            for (auto& b : made) free.push_back(std::move(b));
        }
    } pool;
    uint64_t plain_block_bytes = 0;  // set by block_bytes_for(): the ingest block size of plain input
    std::function<void()> all_emitted;  // called once the last batch has been handed to emit, before the input is closed
    auto produce = [&](uint64_t batch_reads, const std::function<bool(std::unique_ptr<ReadBlock>)>& emit) -> bool {
        auto w = pool.get();
        uint64_t skipped = 0;
        auto full = [&] { return w->n() >= batch_reads || w->bases.size() >= (1ull << 30); };
        mtsv_ingest::ParallelFastx par;
        mtsv_ingest::GzFastx gzpar;  // gzip input: parallel inflate + the same block parsers (MTSV_SERIAL_GZIP=1: zlib's one stream)
        bool use_gz = false;
        // inflating is the expensive part of gzip input: more helpers than plain text needs (measured: 8 threads 3.3 M
        // reads/s, 16 5.5, 32 5.7 against 1.3 on zlib's one stream)
        // (-t / --threads bounds it like every other host-side pool; MTSV_GZ_THREADS=16 is what the 9.0 M reads/s were measured with)
        unsigned gz_threads = host_threads;
        if (const char* e = getenv("MTSV_GZ_THREADS")) gz_threads = (unsigned)std::max(1, atoi(e));
        gz_threads = std::min(gz_threads, std::max(1u, std::thread::hardware_concurrency()));
        // Plain input is cut into blocks of about one batch of reads each (bytes per record estimated from the file's
        // head): a parsed block then IS the batch -- its bases lie in page-locked memory (byte_alloc) that the copy
        // engine reads in place, and the producer thread hands it on without touching the bases again.
        uint64_t ingest_block = 16ull << 20;
        if (getenv("MTSV_INGEST_BLOCK")) ingest_block = strtoull(getenv("MTSV_INGEST_BLOCK"), nullptr, 10);
        else if (plain_block_bytes) ingest_block = plain_block_bytes;
        else if (FILE* hf = fopen(input.c_str(), "rb")) {
            std::vector<char> head(256 << 10);
            const size_t got = fread(head.data(), 1, head.size(), hf);
            fclose(hf);
            uint64_t recs = 0;
            if (got >= 2 && !((uint8_t)head[0] == 0x1f && (uint8_t)head[1] == 0x8b)) {
                if (fastq) {
                    uint64_t lines = 0;
                    for (size_t i = 0; i < got; i++) lines += head[i] == '\n';
                    recs = lines / 4;
                } else {
                    for (size_t i = 0; i < got; i++) recs += head[i] == '>' && (i == 0 || head[i - 1] == '\n');
                }
            }
            // (capped at 96 MiB: a parser thread is slower per byte on larger blocks -- 1 Mi-read blocks of 335 MB parsed at a
            //  third of the rate -- and batches beyond that are put together from several blocks as before)
            if (recs >= 8) ingest_block = std::min<uint64_t>(std::max<uint64_t>((uint64_t)((double)got / (double)recs * (double)batch_reads), 4ull << 20), 96ull << 20);
        }
        plain_block_bytes = ingest_block;
        par.prepare = [&pool](ReadBlock& b) {
            auto stocked = pool.get();
            std::swap(b, *stocked);
        };
        bool serial_from_start = getenv("MTSV_SERIAL_INGEST") != nullptr || !par.open(input, fastq, host_threads, ingest_block);
        if (serial_from_start && !getenv("MTSV_SERIAL_INGEST") && !getenv("MTSV_SERIAL_GZIP") && gzpar.open(input, fastq, gz_threads, ingest_block)) {
            use_gz = true;
            serial_from_start = false;
        }
        if (!serial_from_start) {
            auto blk_owner = pool.get();
            uint64_t irregular = 0, direct_emitted = 0;
            for (;;) {
                ReadBlock& blk = *blk_owner;
                auto r = use_gz ? gzpar.next(blk, &irregular) : par.next(blk, &irregular);
                if (r == mtsv_ingest::ParallelFastx::END) break;
                if (r == mtsv_ingest::ParallelFastx::CORRUPT) {  // records of a member whose CRC-32 then failed have been handed out
                    rd.fail("corrupt gzip data (CRC mismatch)");
                    return false;
                }
                if (r == mtsv_ingest::ParallelFastx::IRREGULAR) {
                    logmsg("DEBUG", std::string(use_gz ? "gzip input" : "input") + " is not plain 4-line FASTQ / FASTA (or not decodable in parallel) at byte " + std::to_string(irregular) + "; continuing with the serial reader");
                    if (gzseek(rd.in.f, (z_off_t)irregular, SEEK_SET) < 0) {
                        rd.fail("read error");
                        return false;
                    }
                    serial_from_start = true;  // the serial loop below continues from here
                    break;
                }
                uint64_t from = 0;
                if (skipped < read_offset) {
                    from = std::min<uint64_t>(read_offset - skipped, blk.n());
                    skipped += from;
                }
                // a block of about a batch, nothing pending: the block is the batch
                // (smaller blocks are collected into a batch -- except the first ones of the file, which the parser cuts
                //  short on purpose so that the GPU has work early)
                if (from == 0 && w->n() == 0 && blk.n() && blk.n() <= batch_reads + batch_reads / 2 && blk.bases.size() < (1ull << 30) &&
                    (2 * blk.n() >= batch_reads || direct_emitted < 4)) {
                    direct_emitted++;
                    if (!emit(std::move(blk_owner))) return true;
                    blk_owner = pool.get();
                    continue;
                }
                // cut the block at batch boundaries
                while (from < blk.n()) {
                    const uint64_t room = batch_reads > w->n() ? batch_reads - w->n() : 0;
                    const uint64_t take = std::min<uint64_t>(room, blk.n() - from);
                    w->append(blk, from, from + take);  // records [from, from + take)
                    from += take;
                    if (full()) {
                        if (!emit(std::move(w))) return true;
                        w = pool.get();
                    }
                }
            }
            if (!serial_from_start) {
                if (w->n() && !emit(std::move(w))) return true;
                if (all_emitted) all_emitted();  // before the teardown: unmapping a 10 GB input took 45 ms
                par.close();
                gzpar.close();
                return true;
            }
            par.close();
            gzpar.close();
        }
        Record r;
        while (rd.next(r)) {
            if (skipped < read_offset) {
                skipped++;
                continue;
            }
            mtsv_ingest::push_record(*w, r);
            if (full()) {
                if (!emit(std::move(w))) return true;
                w = pool.get();
            }
        }
        if (rd.error) return false;
        if (w->n()) emit(std::move(w));
        if (all_emitted) all_emitted();
        return true;
    };

    if (a.parse_only) {  // ingest self-check: counts and FNV-1a checksums of everything the binner would see
        uint64_t n = 0, nb = 0, hb = 1469598103934665603ull, hi = 1469598103934665603ull, hl = 1469598103934665603ull;
        auto fnv = [](uint64_t& h, const uint8_t* p, uint64_t len) {
            for (uint64_t i = 0; i < len; i++) h = (h ^ p[i]) * 1099511628211ull;
        };
        bool ok = produce(a.batch_reads, [&](std::unique_ptr<ReadBlock> w) {
            n += w->n();
            nb += w->bases.size();
            if (getenv("MTSV_PARSE_NOHASH")) {
                pool.put(std::move(w));
                return true;
            }
            fnv(hb, w->bases.data(), w->bases.size());
            fnv(hi, (const uint8_t*)w->ids.data(), w->ids.size());
            for (uint64_t r = 0; r < w->n(); r++) {
                uint64_t len = w->off[r + 1] - w->off[r];
                fnv(hl, (const uint8_t*)&len, 8);
            }
            return true;
        });
        if (!ok) {
            logmsg("ERROR", "Unable to read from input file: " + rd.err_msg);
            return 12;
        }
        printf("records=%llu bases=%llu bases_fnv=%016llx ids_fnv=%016llx lens_fnv=%016llx\n", (unsigned long long)n,
               (unsigned long long)nb, (unsigned long long)hb, (unsigned long long)hi, (unsigned long long)hl);
        return 0;
    }

    // positional writes from several threads: the result file is written at page-cache speed per thread
    const int out_fd = have_results ? ::open(a.results.c_str(), O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0644) : -1;
    off_t out_pos = out_fd >= 0 ? lseek(out_fd, 0, SEEK_END) : 0;
    if (have_results && out_fd < 0) {
        logmsg("ERROR", "Error running query: cannot open results file " + a.results);
        return 2;
    }
    // the partition files: [0] matched, [1] unmatched (-1: not asked for)
    int part_fd[2] = {-1, -1};
    off_t part_pos[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        const std::string& path = k ? a.unmatched : a.matched;
        if (path.empty()) continue;
        part_fd[k] = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (part_fd[k] < 0) {
            logmsg("ERROR", "Error running query: cannot open " + path);
            return 2;
        }
    }
    // (--merge-on-gpu: the flags come from the merged hits, so the hits are gathered with or without a results file)
    const int match_mode = !partition ? MTSV_MATCH_OFF : (have_results || merged) ? MTSV_MATCH_WITH_HITS : MTSV_MATCH_ONLY;
    logmsg("INFO", "Deserializing candidate filter ...");
    std::vector<std::string> index_paths;
    for (size_t at = 0; at <= a.index.size();) {
        size_t c = a.index.find(',', at);
        if (c == std::string::npos) c = a.index.size();
        if (c > at) index_paths.push_back(a.index.substr(at, c - at));
        at = c + 1;
    }
    if (index_paths.empty()) usage_error("The following required arguments were not provided: --index <INDEX>");
    const bool chunked = index_paths.size() > 1;  // Mode B
    // MTSV_CLI_ASSIGN=1: the default results format is written from assignments -- the smallest edit per read and TaxID,
    // reduced on the device (mtsv_batch_set_assignments, MTSV_ASSIGN_ONLY: no hit crosses to the host) -- where one workspace
    // per worker holds a call's hits: a single index (behind --filter-index: the database's workspace) or the collector of
    // --merge-on-gpu.  The file is the same byte for byte.  --output-format long stays on the hits under this switch.
    // The default is 0 (profiles/README.md r14: the measurement and what it decided).
    bool cli_assign = false;
    if (const char* e = getenv("MTSV_CLI_ASSIGN")) cli_assign = atoi(e) != 0;
    cli_assign = cli_assign && have_results && !long_fmt && (!chunked || merged) && match_mode != MTSV_MATCH_ONLY;
    // MTSV_CLI_ASSIGN_LONG=1: the same for --output-format long -- the workspace in MTSV_GRAIN_LONG, one 24-byte record per read
    // and (TaxID, GI, offset) with the smallest edit, the file written by mtsv_format_assignments_gi, byte for byte the same.
    // A switch of its own: MTSV_CLI_ASSIGN alone leaves long output on the hits.  Default 0, not measured yet.
    bool cli_assign_long = false;
    if (const char* e = getenv("MTSV_CLI_ASSIGN_LONG")) cli_assign_long = atoi(e) != 0;
    cli_assign_long = cli_assign_long && have_results && long_fmt && (!chunked || merged) && match_mode != MTSV_MATCH_ONLY;
    const bool cli_records = cli_assign || cli_assign_long;  // the results file is written from assignment records
    const uint64_t a_rec = cli_assign_long ? sizeof(mtsv_assignment_gi) : sizeof(mtsv_assignment);
    // (both record types begin with the 8-byte read: the one place that relies on it)
    static_assert(offsetof(mtsv_assignment, read) == 0 && offsetof(mtsv_assignment_gi, read) == 0, "records begin with the read");
    auto record_read = [a_rec](uint8_t* records, uint64_t i) -> uint64_t& { return *reinterpret_cast<uint64_t*>(records + i * a_rec); };
    std::vector<std::string> filter_paths;
    for (size_t at = 0; filtered && at <= a.filter_index.size();) {
        size_t c = a.filter_index.find(',', at);
        if (c == std::string::npos) c = a.filter_index.size();
        if (c > at) filter_paths.push_back(a.filter_index.substr(at, c - at));
        at = c + 1;
    }
    if (filtered && filter_paths.empty()) usage_error("The argument '--filter-index <INDEX>' requires a value but none was supplied");
    const size_t n_filters = filter_paths.size();
    // One library call takes every batch that is waiting, up to kGroupReads reads (mtsv_batch_run_host_parts): the device
    // is several times faster on passes of a million reads than on a quarter of that (a pass costs ~2.5 ms before it does
    // any work), while the parser is fastest on blocks of ~80 MB.
    uint64_t kGroupReads = std::max<uint64_t>(a.batch_reads, 1ull << 20);
    if (const char* e = getenv("MTSV_CLI_GROUP_READS")) kGroupReads = std::max<uint64_t>(a.batch_reads, strtoull(e, nullptr, 10));
    const size_t group_max = (size_t)std::min<uint64_t>(32, std::max<uint64_t>(1, kGroupReads / std::max<uint64_t>(a.batch_reads, 1)));
    // Several workers per --devices entry, a workspace of ONE lane each: a call is copy in -> kernels -> hits out, and
    // what overlaps on the device are the calls of different workers (tools/call_stream.py: one worker with the
    // default three lanes 165 M reads/s on megaread calls, three workers of one lane 229 M).
    // (three workers on groups of 1 Mi reads: 0.210 s for 32 M reads twice over; two on 512 Ki: 0.225-0.245 -- since the
    //  parser stopped copying its blocks the workers are what a run waits for)
    size_t workers_per_device = 3;
    if (const char* e = getenv("MTSV_CLI_WORKERS")) workers_per_device = (size_t)std::max(1, std::min(8, atoi(e)));
    // (a small input is through before the extra workspaces have paid for themselves)
    uint64_t input_bytes = 0;
    {
        struct stat st;
        if (stat(input.c_str(), &st) == 0) input_bytes = (uint64_t)st.st_size;
    }
    const bool small_input = input_bytes < (256ull << 20) && !getenv("MTSV_CLI_WORKERS");
    if (small_input) workers_per_device = 1;
    const size_t n_workers = chunked && !merged ? 2 : a.devices.size() * workers_per_device;
    // the length of the input's first read (plain text; 150 otherwise): the workspaces are warmed with reads like it
    uint32_t warm_len = 150;
    if (FILE* hf = fopen(input.c_str(), "rb")) {
        std::vector<char> head(64 << 10);
        const size_t got = fread(head.data(), 1, head.size(), hf);
        fclose(hf);
        if (got >= 2 && !((uint8_t)head[0] == 0x1f && (uint8_t)head[1] == 0x8b)) {
            const char* nl = (const char*)memchr(head.data(), '\n', got);
            if (nl) {
                size_t len = 0;
                for (const char* q = nl + 1; q < head.data() + got && *q != '>' && *q != '+'; q++) len += *q != '\n' && *q != '\r';
                if (len >= 32) warm_len = (uint32_t)std::min<size_t>(len, 1000);
            }
        }
    }
    if (folded) {
        // --fold-on-gpu: one chunk resident at a time.  A super-batch of reads is held on the host, in the (page-locked) blocks
        // the parser filled, each block a PIECE with a fold of its own; per chunk: load, make resident, one workspace in
        // MTSV_ASSIGN_ONLY, per piece upload + run + mtsv_fold_add_run, then the workspace and the index are freed.  After the
        // last chunk a piece's records are its result lines (numbered from 0 within the piece, like its IDs: nothing to offset),
        // its flags split its reads, its report adds to the run's.
        // --fold-prefetch: one loader thread runs mtsv_index_load of chunk c + 1 (after the last chunk: of chunk 0 for the next
        // super-batch, when one is known to follow) while this thread makes chunk c resident, runs it over the pieces and folds.
        // The chunks' uploads then pack on the device (MTSV_DEV_PACK_ON_DEVICE), which the measurement found 8 times faster.
        // Depth 1: at most two host indexes are alive, and still one chunk is resident -- c + 1 goes up after c's workspace
        // and index are freed.  mtsv_last_error is thread-local: the loader hands its message over with its return code, and
        // a chunk that failed to load is reported when its turn comes.  flush() joins the loader on every way out.
        const int dev = a.devices[0];
        const int grain = long_fmt ? MTSV_GRAIN_LONG : MTSV_GRAIN_TAXID;
        const uint64_t piece_reads = a.batch_reads + a.batch_reads / 2;
        const uint64_t piece_bases = std::min<uint64_t>(3ull << 30, std::max<uint64_t>(piece_reads * std::max<uint64_t>(512, 2 * (uint64_t)warm_len), 1 << 22));
        if (!getenv("MTSV_CLI_PAGEABLE") && (uint64_t)a.batch_reads * 320 <= (128ull << 20)) {
            mtsv_ingest::byte_alloc().alloc = [](size_t n) { return mtsv_host_alloc(n); };
            mtsv_ingest::byte_alloc().release = [](void* q) { mtsv_host_free(q); };
        }
        if (!getenv("MTSV_VERIFY")) mtsv_set_default_verify_mode(MTSV_VERIFY_EDIT_FIRST);
        logmsg("INFO", "Beginning queries.");
        struct timespec w0;
        clock_gettime(CLOCK_MONOTONIC, &w0);
        auto now = [] {
            struct timespec t;
            clock_gettime(CLOCK_MONOTONIC, &t);
            return t.tv_sec + t.tv_nsec * 1e-9;
        };
        double t_load = 0, t_resident = 0, t_run = 0, t_fold = 0, t_out = 0, t_loader = 0;
        struct Prefetch {  // the loader's chunk: `chunk` is index_paths.size() when there is none
            std::thread th;
            size_t chunk;
            mtsv_index* ix = nullptr;
            int rc = MTSV_OK;
            std::string err;
            double secs = 0;
        } pre;
        pre.chunk = index_paths.size();
        auto pre_start = [&](size_t c) {
            pre.chunk = c;
            pre.th = std::thread([&pre, &now, path = index_paths[c]] {
                const double t0 = now();
                pre.rc = mtsv_index_load(path.c_str(), &pre.ix);
                if (pre.rc != MTSV_OK) pre.err = mtsv_last_error();
                pre.secs = now() - t0;
            });
        };
        auto pre_join = [&] {
            if (pre.th.joinable()) pre.th.join();
        };
        float fold_device_ms = 0, text_device_ms = 0, dedup_device_ms = 0, expand_device_ms = 0;
        std::vector<std::unique_ptr<ReadBlock>> pieces;
        std::vector<mtsv_fold*> folds;  // one per piece of a super-batch, kept from super-batch to super-batch
        // --dedup: a chunk's run sees the distinct sequences of a piece.  Per chunk and piece the reads go up into an intake
        // workspace, mtsv_batch_take_unique packs the first read of every group of identical reads into the chunk's workspace,
        // and the run is folded into the piece's fold of REPRESENTATIVES; after the last chunk mtsv_fold_expand fans those
        // records out into the piece's fold proper, which everything below is derived from as without the flag.  The map is
        // computed again for every chunk, into the piece's mtsv_dupmap, with the same content every time: hashing the piece
        // once per chunk is the price of keeping no reads resident between chunks (a chunk's index may need that room).
        std::vector<mtsv_fold*> rep_folds;
        std::vector<mtsv_dupmap*> dupmaps;
        uint64_t dedup_reads = 0, dedup_distinct = 0;
        uint64_t super_reads = 0, n_super = 0, reads_done = 0, reads_matched = 0;
        mtsv_taxon_stats* sum = nullptr;
        uint64_t n_sum = 0, report_reads = 0;
        int code = 0;
        auto lib_error = [&] {
            logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
            code = 2;
            return false;
        };
        auto write_all = [&](int fd, const char* q, uint64_t len) {
            uint64_t done = 0;
            while (done < len) {
                const ssize_t r = ::write(fd, q + done, len - done);
                if (r <= 0) return false;
                done += (uint64_t)r;
            }
            return true;
        };
        auto flush = [&](bool more) -> bool {  // the super-batch collected so far, through every chunk; more: another one follows
            if (pieces.empty()) return true;
            struct JoinLoader {  // (no loader thread outlives flush())
                decltype(pre_join)& join;
                ~JoinLoader() { join(); }
            } join_loader{pre_join};
            while (folds.size() < pieces.size()) {
                mtsv_fold* f = nullptr;
                if (mtsv_fold_create(dev, grain, &f) != MTSV_OK) return lib_error();
                folds.push_back(f);
            }
            while (a.dedup && rep_folds.size() < pieces.size()) {
                mtsv_fold* f = nullptr;
                mtsv_dupmap* m = nullptr;
                if (mtsv_fold_create(dev, grain, &f) != MTSV_OK) return lib_error();
                rep_folds.push_back(f);
                if (mtsv_dupmap_create(dev, &m) != MTSV_OK) return lib_error();
                dupmaps.push_back(m);
            }
            for (size_t k = 0; k < pieces.size(); k++)
                if (mtsv_fold_reset(a.dedup ? rep_folds[k] : folds[k], pieces[k]->n()) != MTSV_OK) return lib_error();
            for (size_t c = 0; c < index_paths.size(); c++) {
                mtsv_index* ix = nullptr;
                mtsv_batch *ws = nullptr, *intake = nullptr;
                double t0 = now();
                int rc;
                if (a.fold_prefetch && pre.chunk == c) {  // the loader has it, or is on it: t_load counts the wait
                    pre_join();
                    rc = pre.rc;
                    ix = pre.ix;
                    t_loader += pre.secs;
                    pre.ix = nullptr;
                    pre.chunk = index_paths.size();
                    if (rc != MTSV_OK) {
                        logmsg("ERROR", "Error running query: " + pre.err);
                        code = 2;
                        return false;
                    }
                } else {
                    rc = mtsv_index_load(index_paths[c].c_str(), &ix);
                }
                t_load += now() - t0;
                if (a.fold_prefetch && rc == MTSV_OK) {
                    if (c + 1 < index_paths.size())
                        pre_start(c + 1);
                    else if (more)
                        pre_start(0);
                }
                t0 = now();
                // (under --fold-prefetch the chunk is packed on the device: 63 ms against 527 ms a chunk of 3.45e8 symbols,
                //  profiles/README.md r18; without the flag the upload is the one it was)
                if (rc == MTSV_OK) rc = mtsv_index_to_device(ix, dev, a.fold_prefetch ? MTSV_DEV_PACK_ON_DEVICE : MTSV_DEV_DEFAULT);
                t_resident += now() - t0;
                if (rc == MTSV_OK) rc = mtsv_batch_create_lanes(ix, dev, piece_reads, piece_bases, 0, 1, &ws);
                if (rc == MTSV_OK) rc = mtsv_batch_set_assignment_grain(ws, grain);
                if (rc == MTSV_OK) rc = mtsv_batch_set_assignments(ws, MTSV_ASSIGN_ONLY);
                if (rc == MTSV_OK && a.dedup) rc = mtsv_batch_create_lanes(ix, dev, piece_reads, piece_bases, 1, 1, &intake);  // (it never runs)
                for (size_t k = 0; k < pieces.size() && rc == MTSV_OK; k++) {
                    const ReadBlock& rb = *pieces[k];
                    t0 = now();
                    rc = mtsv_batch_upload(a.dedup ? intake : ws, rb.bases.data(), rb.off.data(), rb.n());
                    if (rc == MTSV_OK && a.dedup) {
                        uint64_t n_distinct = 0, bases_kept = 0;
                        float ms = 0;
                        rc = mtsv_batch_take_unique(ws, intake, dupmaps[k], &n_distinct, &bases_kept, &ms);
                        dedup_device_ms += ms;
                        if (rc == MTSV_OK && c == 0) {
                            dedup_reads += rb.n();
                            dedup_distinct += n_distinct;
                        }
                    }
                    if (rc == MTSV_OK) rc = mtsv_batch_run(ws, &p);
                    t_run += now() - t0;
                    t0 = now();
                    float ms = 0;
                    if (rc == MTSV_OK) rc = mtsv_fold_add_run(a.dedup ? rep_folds[k] : folds[k], ws, &ms);
                    fold_device_ms += ms;
                    t_fold += now() - t0;
                }
                if (rc != MTSV_OK) lib_error();  // (before the frees: the message is the failing call's)
                mtsv_batch_free(ws);
                mtsv_batch_free(intake);
                mtsv_index_free(ix);
                if (rc != MTSV_OK) return false;
                logmsg("DEBUG", "chunk " + index_paths[c] + " folded into " + std::to_string(pieces.size()) + " pieces");
            }
            const double t0 = now();
            for (size_t k = 0; k < pieces.size(); k++) {
                ReadBlock& rb = *pieces[k];
                mtsv_fold* f = folds[k];
                if (a.dedup) {  // (the piece's map is the last chunk's, equal to every chunk's)
                    float ms = 0;
                    if (mtsv_fold_expand(f, rep_folds[k], dupmaps[k], &ms) != MTSV_OK) return lib_error();
                    expand_device_ms += ms;
                }
                if (out_fd >= 0) {
                    void* recs = nullptr;
                    uint64_t n_recs = 0;
                    char* text = nullptr;
                    uint64_t len = 0;
                    int rc = MTSV_OK;
                    if (a.text_gpu) {  // (--text-on-gpu: the lines are written where the records are)
                        float ms = 0;
                        rc = mtsv_fold_format_text(f, rb.ids.data(), rb.id_off.data(), rb.n(), &text, &len, &ms);
                        text_device_ms += ms;
                    } else {
                        rc = long_fmt ? mtsv_fold_download_gi(f, (mtsv_assignment_gi**)&recs, &n_recs) : mtsv_fold_download(f, (mtsv_assignment**)&recs, &n_recs);
                    }
                    if (rc == MTSV_OK && !a.text_gpu)
                        rc = long_fmt ? mtsv_format_assignments_gi((const mtsv_assignment_gi*)recs, n_recs, rb.ids.data(), rb.id_off.data(), rb.n(), &text, &len)
                                      : mtsv_format_assignments((const mtsv_assignment*)recs, n_recs, rb.ids.data(), rb.id_off.data(), rb.n(), &text, &len);
                    if (rc != MTSV_OK) lib_error();
                    mtsv_free(recs);
                    const bool written = rc == MTSV_OK && write_all(out_fd, text, len);
                    mtsv_free(text);
                    if (rc != MTSV_OK) return false;
                    if (!written) {
                        logmsg("ERROR", "Error writing to result file");
                        code = 11;
                        return false;
                    }
                }
                if (!a.report.empty()) {
                    mtsv_taxon_stats *rows = nullptr, *both = nullptr;
                    uint64_t n_rows = 0, n_both = 0, reads = 0;
                    const bool ok = mtsv_fold_taxa_report(f, &rows, &n_rows, &reads, nullptr) == MTSV_OK &&
                                    mtsv_merge_taxa_reports(sum, n_sum, rows, n_rows, &both, &n_both) == MTSV_OK;
                    if (!ok) lib_error();
                    mtsv_free(rows);
                    if (!ok) return false;
                    mtsv_free(sum);
                    sum = both;
                    n_sum = n_both;
                    report_reads += reads;
                }
                if (partition) {
                    uint64_t *words = nullptr, n_flagged = 0, n_match = 0;
                    if (mtsv_fold_match_flags(f, &words, &n_flagged, &n_match) != MTSV_OK) return lib_error();
                    std::string side[2];
                    for (uint64_t i = 0; i < rb.n(); i++) {
                        const int sd = (words[i >> 6] >> (i & 63)) & 1 ? 0 : 1;
                        if (part_fd[sd] >= 0) mtsv_ingest::write_block_record(side[sd], fastq, rb, i);
                    }
                    mtsv_free(words);
                    reads_matched += n_match;
                    for (int sd = 0; sd < 2; sd++)
                        if (part_fd[sd] >= 0 && !write_all(part_fd[sd], side[sd].data(), side[sd].size())) {
                            logmsg("ERROR", std::string("Error writing to ") + (sd ? a.unmatched : a.matched));
                            code = 11;
                            return false;
                        }
                }
                reads_done += rb.n();
                pool.put(std::move(pieces[k]));
            }
            t_out += now() - t0;
            pieces.clear();
            super_reads = 0;
            n_super++;
            logmsg("DEBUG", "taxonomic binning: " + std::to_string(reads_done) + " reads done");
            return true;
        };
        auto take_piece = [&](std::unique_ptr<ReadBlock> rb) {
            if (rb->n() > piece_reads || rb->bases.size() > piece_bases) {
                logmsg("ERROR", "Error running query: a batch of reads holds more than " + std::to_string(piece_reads) + " reads or " + std::to_string(piece_bases) +
                                    " bases, which the chunks' workspaces are sized for: give a smaller --batch-reads");
                code = 2;
                return false;
            }
            if (!pieces.empty() && super_reads + rb->n() > a.fold_reads && !flush(true)) return false;
            super_reads += rb->n();
            pieces.push_back(std::move(rb));
            return true;
        };
        const bool parsed = produce(std::min<uint64_t>(a.batch_reads, a.fold_reads), [&](std::unique_ptr<ReadBlock> rb) {
            // (the parser hands out blocks of up to one and a half batches: a super-batch holds at most --fold-reads reads)
            if (rb->n() <= a.fold_reads) return take_piece(std::move(rb));
            for (uint64_t from = 0; from < rb->n(); from += a.fold_reads) {
                auto part = pool.get();
                part->append(*rb, from, std::min<uint64_t>(from + a.fold_reads, rb->n()));
                if (!take_piece(std::move(part))) return false;
            }
            pool.put(std::move(rb));
            return true;
        });
        // every way out of the folded run ends alike: the process leaves at once, or (MTSV_CLI_CLEAN_EXIT=1) frees what it holds
        auto leave = [&](int c) {
            mtsv_free(sum);
            sum = nullptr;
            pre_join();  // (joined by flush() already; a chunk it loaded for a super-batch that never came is freed below)
            if (!getenv("MTSV_CLI_CLEAN_EXIT")) {
                fflush(nullptr);
                _exit(c);
            }
            for (auto* f : folds) mtsv_fold_free(f);
            folds.clear();
            for (auto* f : rep_folds) mtsv_fold_free(f);
            rep_folds.clear();
            for (auto* m : dupmaps) mtsv_dupmap_free(m);
            dupmaps.clear();
            mtsv_index_free(pre.ix);
            pre.ix = nullptr;
            return c;
        };
        if (!parsed && !code) {
            logmsg("ERROR", "Unable to read from input file: " + rd.err_msg);
            code = 12;  // binner.rs:81-84
        }
        if (!code) flush(false);
        if (code) return leave(code);
        if (out_fd >= 0 && ::close(out_fd) != 0) {
            logmsg("ERROR", "Error writing to result file");
            return leave(11);
        }
        for (int k = 0; k < 2; k++)
            if (part_fd[k] >= 0 && ::close(part_fd[k]) != 0) {
                logmsg("ERROR", std::string("Error writing to ") + (k ? a.unmatched : a.matched));
                return leave(11);
            }
        if (partition)
            logmsg("INFO", "Partitioned " + std::to_string(reads_done) + " reads: " + std::to_string(reads_matched) + " matched, " + std::to_string(reads_done - reads_matched) +
                               " unmatched.");
        if (a.dedup) logmsg("INFO", "Collapsed " + std::to_string(dedup_reads) + " reads to " + std::to_string(dedup_distinct) + " distinct sequences.");
        if (!a.report.empty()) {
            char* text = nullptr;
            uint64_t text_len = 0;
            if (mtsv_format_taxa_report(sum, n_sum, report_reads, &text, &text_len) != MTSV_OK) {
                logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
                return leave(2);
            }
            FILE* rf = fopen(a.report.c_str(), "wb");
            const bool written = rf && fwrite(text, 1, text_len, rf) == text_len;
            if ((rf && fclose(rf) != 0) || !written) {
                logmsg("ERROR", "Error writing to taxa report file");
                return leave(11);
            }
            mtsv_free(text);
        }
        struct timespec w1;
        clock_gettime(CLOCK_MONOTONIC, &w1);
        char msg[160];
        snprintf(msg, sizeof msg, "All worker and result consumer threads terminated. Took %.3f seconds.", (w1.tv_sec - w0.tv_sec) + (w1.tv_nsec - w0.tv_nsec) * 1e-9);
        logmsg("INFO", msg);
        // MTSV_CLI_TIMING=1: where a folded run spends its time (seconds; tools/fold_ab.py reads this line)
        // (--fold-prefetch: index_load is the time this thread waited for the loader -- and the first chunk's load -- and the
        //  loader's own time, which ran beside the other figures, follows)
        char prefetch_note[96] = "";
        if (a.fold_prefetch) snprintf(prefetch_note, sizeof prefetch_note, "; prefetch: loader %.3f s, waited_for_loader %.3f s", t_loader, t_load);
        if (getenv("MTSV_CLI_TIMING"))
            fprintf(stderr, "[cli fold timing] super_batches %llu chunks %zu reads %llu; index_load %.3f s, index_to_device %.3f s, upload_and_run %.3f s, fold %.3f s "
                            "(device %.3f ms), results_report_flags %.3f s%s\n",
                    (unsigned long long)n_super, index_paths.size(), (unsigned long long)reads_done, t_load, t_resident, t_run, t_fold, fold_device_ms, t_out,
                    prefetch_note);
        if (getenv("MTSV_CLI_TIMING") && a.text_gpu) fprintf(stderr, "[cli text timing] text_on_gpu device %.3f ms\n", text_device_ms);
        if (getenv("MTSV_CLI_TIMING") && a.dedup)
            fprintf(stderr, "[cli dedup timing] take_unique device %.3f ms, expand device %.3f ms\n", dedup_device_ms, expand_device_ms);
        return leave(0);
    }
    // (batches too large for one parser block are put together from several blocks by appending: those stay in ordinary
    //  memory -- growing a page-locked buffer means allocating another one -- and are staged by the library)
    std::thread stock_thread;
    struct Joiner {  // (an early return must not leave the thread running)
        std::thread& t;
        ~Joiner() {
            if (t.joinable()) t.join();
        }
    } stock_joiner{stock_thread};
    if (!getenv("MTSV_CLI_PAGEABLE") && (uint64_t)a.batch_reads * 320 <= (128ull << 20)) {
        mtsv_ingest::byte_alloc().alloc = [](size_t n) { return mtsv_host_alloc(n); };
        mtsv_ingest::byte_alloc().release = [](void* q) { mtsv_host_free(q); };
        // stock: the parser's window of blocks plus what sits in the queues and with the workers
        if (const char* e = getenv("MTSV_INGEST_BLOCK")) plain_block_bytes = strtoull(e, nullptr, 10);
        const uint64_t est = plain_block_bytes ? plain_block_bytes : (uint64_t)a.batch_reads * 320;
        const uint64_t per_call = std::min<uint64_t>(8, std::max<uint64_t>(1, std::max<uint64_t>(a.batch_reads, 1ull << 20) / std::max<uint64_t>(a.batch_reads, 1)));
        // (on a thread of its own: ~2 GB of page-locked memory take 0.1 s to create, the index is loaded meanwhile)
        const size_t n_stock = small_input ? 8 : std::min<size_t>(2 * host_threads + 2 + (size_t)(2 * per_call + 1) * (n_workers + 1), 128);
        const uint64_t stock_bytes = std::min<uint64_t>(est / 2 + (1 << 20), 512ull << 20);
        stock_thread = std::thread([&pool, n_stock, stock_bytes] { pool.stock(n_stock, stock_bytes); });
    }
    // The library would pack the bases to 4-bit codes on the host before they cross PCIe (host_pack.hpp: a dozen threads);
    // here the parser's threads need the CPUs and the link is not what bounds a run: the blocks go as they are
    // (MTSV_CLI_PACKED=1: packed).
    if (!getenv("MTSV_CLI_PACKED")) setenv("MTSV_H2D_PLAIN", "1", 0);
    // the two acceptance predicates are evaluated edit distance first (identical hits, about twice the device
    // rate for reads up to 253 bases); MTSV_VERIFY=reference keeps the reference's order
    if (!getenv("MTSV_VERIFY")) mtsv_set_default_verify_mode(MTSV_VERIFY_EDIT_FIRST);
    std::vector<mtsv_index*> idx(index_paths.size(), nullptr);
    std::vector<int> chunk_dev(index_paths.size(), 0);
    for (size_t c = 0; c < index_paths.size(); c++) {
        chunk_dev[c] = a.devices[c % a.devices.size()];
        if (mtsv_index_load(index_paths[c].c_str(), &idx[c]) != MTSV_OK) {
            logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
            return 2;
        }
        // one index: resident on every listed device; chunks: chunk c on its device
        for (size_t d = 0; d < (chunked ? 1 : a.devices.size()); d++)
            if (mtsv_index_to_device(idx[c], chunked ? chunk_dev[c] : a.devices[d], MTSV_DEV_DEFAULT) != MTSV_OK) {
                logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
                return 2;
            }
    }
    // the filter indexes: every one resident on every listed device, beside the database
    std::vector<mtsv_index*> fidx(n_filters, nullptr);
    for (size_t c = 0; c < n_filters; c++) {
        if (mtsv_index_load(filter_paths[c].c_str(), &fidx[c]) != MTSV_OK) {
            logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
            return 2;
        }
        for (size_t d = 0; d < a.devices.size(); d++)
            if (mtsv_index_to_device(fidx[c], a.devices[d], MTSV_DEV_DEFAULT) != MTSV_OK) {
                logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
                return 2;
            }
    }
    setup_mark("index loaded and resident");
    // the workers' workspaces (one index): part of the device set-up, like making the index resident -- created, sized for
    // the calls to come and run once on reads sampled from the index (mtsv_batch_reserve_host)
    std::vector<mtsv_batch*> ws_ready(chunked && !merged ? 0 : n_workers, nullptr);
    // --merge-on-gpu: a workspace per worker and chunk, which hold a call's reads as a resident batch (the first by upload, the
    // others by mtsv_batch_copy_reads); ws_ready[wk] is the worker's collector, which mtsv_batch_merge_runs fills and the
    // report and the flags are read from.  A call is one block of reads.
    std::vector<std::vector<mtsv_batch*>> cws(merged ? n_workers : 0, std::vector<mtsv_batch*>(index_paths.size(), nullptr));
    const uint64_t merge_reads = a.batch_reads + a.batch_reads / 2;
    const uint64_t merge_bases = std::min<uint64_t>(3ull << 30, std::max<uint64_t>(merge_reads * std::max<uint64_t>(512, 2 * (uint64_t)warm_len), 1 << 22));
    // --filter-index: a workspace per worker and filter stage.  The first takes the host batch; the later ones and the
    // database's receive their reads in HBM (mtsv_batch_take_reads) and hold them as a resident batch, so they are created
    // with room for the bases of a call: chain_bases (a call whose blocks hold more is cut into several).
    std::vector<std::vector<mtsv_batch*>> fws(ws_ready.size(), std::vector<mtsv_batch*>(n_filters, nullptr));
    const uint64_t chain_reads = kGroupReads + a.batch_reads + a.batch_reads / 2;
    const uint64_t chain_bases = std::min<uint64_t>(3ull << 30, chain_reads * std::max<uint64_t>(512, 2 * (uint64_t)warm_len));
    {
        std::vector<int> ws_rc(ws_ready.size(), MTSV_OK);
        std::vector<std::string> ws_msg(ws_ready.size());
        auto make_ws = [&](size_t wk) {
            const uint64_t call_reads = kGroupReads + a.batch_reads + a.batch_reads / 2;
            const int dev = a.devices[wk % a.devices.size()];
            // (a workspace that receives its reads from a filter stage runs them as one resident batch: room for all of them)
            auto create = [&](mtsv_index* ix, bool resident, mtsv_batch** out) {
                const uint64_t ws_bases = resident ? chain_bases : 1 << 22;
                return workers_per_device > 1 ? mtsv_batch_create_lanes(ix, dev, call_reads, ws_bases, 0, 1, out)
                                              : mtsv_batch_create(ix, dev, resident ? call_reads : mtsv_bin_batch_workspace_reads(call_reads), ws_bases, 0, out);
            };
            const bool warm = !small_input && !getenv("MTSV_CLI_COLD");
            if (merged) {
                int rc = mtsv_batch_create_lanes(idx[0], dev, 1024, 1 << 16, 0, 1, &ws_ready[wk]);
                for (size_t c = 0; c < idx.size() && rc == MTSV_OK; c++) {
                    rc = mtsv_batch_create_lanes(idx[c], dev, merge_reads, merge_bases, 0, 1, &cws[wk][c]);
                    if (rc == MTSV_OK && warm) rc = mtsv_batch_reserve_host(cws[wk][c], 4096, 4096 * (uint64_t)(warm_len + warm_len / 8), warm_len);
                }
                if (rc == MTSV_OK && !a.report.empty()) rc = mtsv_batch_set_taxa_report(ws_ready[wk], 1);
                if (rc == MTSV_OK && partition) rc = mtsv_batch_set_match_flags(ws_ready[wk], match_mode);
                if (rc == MTSV_OK && cli_assign_long) rc = mtsv_batch_set_assignment_grain(ws_ready[wk], MTSV_GRAIN_LONG);
                if (rc == MTSV_OK && cli_records) rc = mtsv_batch_set_assignments(ws_ready[wk], MTSV_ASSIGN_ONLY);
                ws_rc[wk] = rc;
                if (rc != MTSV_OK) ws_msg[wk] = mtsv_last_error();  // (thread-local)
                return;
            }
            int rc = create(idx[0], filtered, &ws_ready[wk]);
            // (only the workspace that takes the host batches needs their arenas; the others are warmed on a small batch)
            if (rc == MTSV_OK && warm)
                rc = filtered ? mtsv_batch_reserve_host(ws_ready[wk], 4096, 4096 * (uint64_t)(warm_len + warm_len / 8), warm_len)
                              : mtsv_batch_reserve_host(ws_ready[wk], call_reads, call_reads * (uint64_t)(warm_len + warm_len / 8), warm_len);
            for (size_t k = 0; k < n_filters && rc == MTSV_OK; k++) {
                rc = create(fidx[k], k > 0, &fws[wk][k]);
                if (rc == MTSV_OK && warm)
                    rc = k ? mtsv_batch_reserve_host(fws[wk][k], 4096, 4096 * (uint64_t)(warm_len + warm_len / 8), warm_len)
                           : mtsv_batch_reserve_host(fws[wk][k], call_reads, call_reads * (uint64_t)(warm_len + warm_len / 8), warm_len);
                if (rc == MTSV_OK) rc = mtsv_batch_set_match_flags(fws[wk][k], MTSV_MATCH_ONLY);  // (after the warm-up reads)
            }
            if (rc == MTSV_OK && !a.report.empty()) rc = mtsv_batch_set_taxa_report(ws_ready[wk], 1);  // (after the warm-up reads)
            if (rc == MTSV_OK && partition) rc = mtsv_batch_set_match_flags(ws_ready[wk], match_mode);
            if (rc == MTSV_OK && cli_assign_long) rc = mtsv_batch_set_assignment_grain(ws_ready[wk], MTSV_GRAIN_LONG);
            if (rc == MTSV_OK && cli_records) rc = mtsv_batch_set_assignments(ws_ready[wk], MTSV_ASSIGN_ONLY);  // (after the warm-up reads)
            ws_rc[wk] = rc;
            if (rc != MTSV_OK) ws_msg[wk] = mtsv_last_error();  // (thread-local)
        };
        std::vector<std::thread> th;
        for (size_t wk = 1; wk < ws_ready.size(); wk++) th.emplace_back(make_ws, wk);
        if (!ws_ready.empty()) make_ws(0);
        for (auto& t : th) t.join();
        for (size_t wk = 0; wk < ws_ready.size(); wk++)
            if (ws_rc[wk] != MTSV_OK) {
                logmsg("ERROR", "Error running query: " + ws_msg[wk]);
                return 2;
            }
    }
    setup_mark("workspaces ready");
    // parsed blocks land in page-locked memory from here on: the GPU copies them from where the parser put them
    if (stock_thread.joinable()) stock_thread.join();
    setup_mark("stock of page-locked blocks ready");
    logmsg("INFO", "Beginning queries.");
    struct timespec w0;
    clock_gettime(CLOCK_MONOTONIC, &w0);
    // MTSV_CLI_TIMING=1: where the stages of the command line spend their time (seconds, summed per stage)
    const bool cli_timing = getenv("MTSV_CLI_TIMING") != nullptr;
    auto now = [] {
        struct timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return t.tv_sec + t.tv_nsec * 1e-9;
    };
    std::atomic<uint64_t> t_ingest_wait{0}, t_push_wait{0}, t_gpu{0}, t_gpu_wait{0}, t_fmt{0}, t_done_wait{0}, t_write_wait{0};
    auto acc = [](std::atomic<uint64_t>& a, double s) { a.fetch_add((uint64_t)(s * 1e6)); };
    const double t_begin = now();
    std::mutex marks_mu;
    std::vector<std::pair<std::string, double>> marks;  // (what, seconds since the queries began), printed with the timing
    auto mark = [&](const std::string& what) {
        if (!cli_timing) return;
        std::lock_guard<std::mutex> lk(marks_mu);
        marks.emplace_back(what, now() - t_begin);
    };

    // Overlapped stages (the reference overlaps producer / workers / joiner the same way,
    // vendor/cue/src/lib.rs:45-105): the producer parses FASTX into numbered batches, GPU workers (one per
    // --devices entry; two dispatchers over all chunks in chunk mode) take batches as they come, a writer
    // thread formats and writes the result lines in input order.
    struct Work {
        std::unique_ptr<ReadBlock> rb;
        uint64_t seq = 0;
        mtsv_hit* hits = nullptr;  // this batch's hits: a slice of the array hits_owner holds (read numbers: the call's, read_first + the batch's)
        uint64_t n_hits = 0;
        uint64_t read_first = 0;  // the batch's first read in the numbering of its call (the formatter subtracts it)
        std::shared_ptr<void> hits_owner;  // the result array of the library call the batch was part of
        // MTSV_CLI_ASSIGN=1, MTSV_CLI_ASSIGN_LONG=1: the batch's assignments instead (the same slicing and numbering; records of
        // a_rec bytes that begin with the read), and their array
        uint8_t* assigns = nullptr;
        uint64_t n_assigns = 0;
        std::shared_ptr<void> assigns_owner;
        std::shared_ptr<uint64_t> flags;   // --matched / --unmatched: the match flags of that call; read i of the batch is bit read_first + i
    };
    struct Queue {
        std::mutex mu;
        std::condition_variable cv;
        std::deque<std::unique_ptr<Work>> q;
        bool closed = false;
        size_t cap = 2;
        size_t n_takers = 1;  // threads that call pop_group
        void push(std::unique_ptr<Work> w) {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return q.size() < cap || closed; });
            q.push_back(std::move(w));
            cv.notify_all();
        }
        // the next batches in order, up to max_reads reads / max_n batches: a full group, or -- when the input has ended or
        // `idle` says that the device has nothing else to do -- whatever is waiting
        // (max_bases: a group holds at most that many bases -- or one batch)
        std::vector<std::unique_ptr<Work>> pop_group(uint64_t max_reads, size_t max_n, const std::function<bool()>& idle, uint64_t max_bases = ~0ull) {
            std::unique_lock<std::mutex> lk(mu);
            auto waiting = [&] {
                uint64_t r = 0;
                for (auto& w : q) r += w->rb->n();
                return r;
            };
            for (;;) {
                if (!q.empty() && (closed || q.size() >= max_n || waiting() >= max_reads || idle())) break;
                if (q.empty() && closed) return {};
                cv.wait_for(lk, std::chrono::microseconds(200));  // (idle() changes without a notification)
            }
            // (the input has ended: what is left is shared out, so that the workers finish together)
            if (closed && n_takers > 1) max_n = std::min(max_n, (q.size() + n_takers - 1) / n_takers);
            std::vector<std::unique_ptr<Work>> g;
            uint64_t r = 0, nb = 0;
            while (!q.empty() && g.size() < max_n && r < max_reads) {
                nb += q.front()->rb->bases.size();
                if (!g.empty() && nb > max_bases) break;
                r += q.front()->rb->n();
                g.push_back(std::move(q.front()));
                q.pop_front();
            }
            cv.notify_all();
            return g;
        }
        std::unique_ptr<Work> try_pop() {  // nullptr when nothing is waiting
            std::lock_guard<std::mutex> lk(mu);
            if (q.empty()) return nullptr;
            auto w = std::move(q.front());
            q.pop_front();
            cv.notify_all();
            return w;
        }
        std::unique_ptr<Work> pop() {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !q.empty() || closed; });
            if (q.empty()) return nullptr;
            auto w = std::move(q.front());
            q.pop_front();
            cv.notify_all();
            return w;
        }
        void close() {
            std::lock_guard<std::mutex> lk(mu);
            closed = true;
            cv.notify_all();
        }
    };
    Queue parsed, done;
    parsed.cap = (n_workers + 1) * group_max + 1;
    parsed.n_takers = n_workers;
    done.cap = n_workers * group_max + 1;
    std::atomic<int> calls_in_flight{0};
    std::atomic<uint64_t> reads_matched{0}, reads_partitioned{0};
    std::vector<std::atomic<uint64_t>> stage_in(n_filters), stage_removed(n_filters);  // --filter-index: reads into / dropped by each stage
    for (size_t k = 0; k < n_filters; k++) stage_in[k] = 0, stage_removed[k] = 0;
    std::mutex err_mu;
    int exit_code = 0;
    auto set_code = [&](int c) {
        std::lock_guard<std::mutex> lk(err_mu);
        if (!exit_code) exit_code = c;
    };
    auto failed = [&] {
        std::lock_guard<std::mutex> lk(err_mu);
        return exit_code != 0;
    };

    uint64_t n_batches = 0;
    all_emitted = [&] {
        mark("last block parsed");
        parsed.close();
    };
    std::thread reader([&] {
        double t_last = now();
        bool ok = produce(a.batch_reads, [&](std::unique_ptr<ReadBlock> rb) {
            if (failed()) return false;
            auto w = std::make_unique<Work>();
            w->rb = std::move(rb);
            w->seq = n_batches++;
            const double t_a = now();
            if (w->seq == 0) mark("first block parsed");
            acc(t_ingest_wait, t_a - t_last);  // producing this batch (mostly: waiting for the parser threads)
            parsed.push(std::move(w));
            t_last = now();
            acc(t_push_wait, t_last - t_a);    // waiting for room in the queue to the GPU workers
            return true;
        });
        if (!ok) {
            logmsg("ERROR", "Unable to read from input file: " + rd.err_msg);
            set_code(12);  // binner.rs:81-84
        }
        parsed.close();
        mark("reader done");
    });

    // helper threads of the result side: the formatting of a batch's hits runs on them in parallel, and the
    // finished text of batch k is written (positional writes at offsets fixed in batch order) while batch k+1
    // is being formatted
    struct Helpers {
        std::mutex mu;
        std::condition_variable cv, idle;
        std::deque<std::function<void()>> q;
        std::vector<std::thread> th;
        size_t running = 0;
        bool stop = false;
        explicit Helpers(unsigned n) {
            for (unsigned i = 0; i < n; i++)
                th.emplace_back([this] {
                    for (;;) {
                        std::function<void()> f;
                        {
                            std::unique_lock<std::mutex> lk(mu);
                            cv.wait(lk, [&] { return stop || !q.empty(); });
                            if (q.empty()) return;
                            f = std::move(q.front());
                            q.pop_front();
                            running++;
                        }
                        f();
                        {
                            std::lock_guard<std::mutex> lk(mu);
                            running--;
                        }
                        idle.notify_all();
                    }
                });
        }
        void submit(std::function<void()> f) {
            {
                std::lock_guard<std::mutex> lk(mu);
                q.push_back(std::move(f));
            }
            cv.notify_one();
        }
        void wait_all() {
            std::unique_lock<std::mutex> lk(mu);
            idle.wait(lk, [&] { return q.empty() && running == 0; });
        }
        void wait_below(size_t n) {  // until fewer than n jobs are queued or running
            std::unique_lock<std::mutex> lk(mu);
            idle.wait(lk, [&] { return q.size() + running < n; });
        }
        ~Helpers() {
            {
                std::lock_guard<std::mutex> lk(mu);
                stop = true;
            }
            cv.notify_all();
            for (auto& t : th) t.join();
        }
    };
    Helpers fmt_pool(host_threads), write_pool(std::max(2u, host_threads / 2));
    std::atomic<bool> write_failed{false};
    std::thread writer([&] {
        uint64_t total = 0, next_seq = 0;
        std::vector<std::unique_ptr<Work>> held;  // batches that finished ahead of their turn
        for (;;) {
            std::unique_ptr<Work> w;
            for (auto& h : held)
                if (h && h->seq == next_seq) {
                    w = std::move(h);
                    h = std::move(held.back());
                    held.pop_back();
                    break;
                }
            if (!w) {
                const double t_a = now();
                w = done.pop();
                acc(t_done_wait, now() - t_a);
                if (!w) break;
                if (w->seq != next_seq) {
                    held.push_back(std::move(w));
                    continue;
                }
            }
            next_seq++;
            const double t_f0 = now();
            // write_assignments over slices of the batch's hits (cut between reads), one thread each
            const uint64_t n_reads = w->rb->n();
            const uint64_t n_items = cli_records ? w->n_assigns : w->n_hits;
            auto read_of = [&](uint64_t i) { return cli_records ? record_read(w->assigns, i) : w->hits[i].read; };
            const unsigned parts = n_items >= (1u << 16) ? host_threads : 1;
            std::vector<uint64_t> cut(parts + 1, n_items);
            cut[0] = 0;
            for (unsigned k = 1; k < parts; k++) {
                uint64_t c = std::max(cut[k - 1], n_items * k / parts);
                while (c > cut[k - 1] && c < n_items && read_of(c) == read_of(c - 1)) c++;
                cut[k] = c;
            }
            // --matched / --unmatched: the batch's records, each to its side, serialised over ranges of reads in parallel and
            // written at offsets fixed in batch order, like the result lines
            if (partition && w->flags && !failed() && !write_failed.load()) {
                const unsigned pp = n_reads >= (1u << 14) ? host_threads : 1;
                std::vector<std::string> side[2];
                side[0].resize(pp);
                side[1].resize(pp);
                const ReadBlock& blk = *w->rb;
                const uint64_t* fw = w->flags.get();
                const uint64_t first = w->read_first;
                const bool want[2] = {part_fd[0] >= 0, part_fd[1] >= 0};
                auto ser = [&](unsigned k) {
                    const uint64_t r0 = n_reads * k / pp, r1 = n_reads * (k + 1) / pp;
                    for (int sd = 0; sd < 2; sd++)
                        if (want[sd]) side[sd][k].reserve((size_t)((blk.off[r1] - blk.off[r0]) * (fastq ? 2 : 1) + (r1 - r0) * 48));
                    for (uint64_t i = r0; i < r1; i++) {
                        const uint64_t bit = first + i;
                        const int sd = (fw[bit >> 6] >> (bit & 63)) & 1 ? 0 : 1;
                        if (want[sd]) mtsv_ingest::write_block_record(side[sd][k], fastq, blk, i);
                    }
                };
                if (pp > 1) {
                    for (unsigned k = 1; k < pp; k++) fmt_pool.submit([&ser, k] { ser(k); });
                    ser(0);
                    fmt_pool.wait_all();
                } else {
                    ser(0);
                }
                for (int sd = 0; sd < 2; sd++)
                    for (unsigned k = 0; k < pp && want[sd]; k++) {
                        if (side[sd][k].empty()) continue;
                        auto tx = std::make_shared<std::string>(std::move(side[sd][k]));
                        const off_t at = part_pos[sd];
                        part_pos[sd] += (off_t)tx->size();
                        const int fd = part_fd[sd];
                        write_pool.submit([tx, at, fd, &write_failed, &set_code] {
                            uint64_t done = 0;
                            while (done < tx->size()) {
                                ssize_t r = pwrite(fd, tx->data() + done, tx->size() - done, at + (off_t)done);
                                if (r <= 0) {
                                    write_failed.store(true);
                                    set_code(11);
                                    break;
                                }
                                done += (uint64_t)r;
                            }
                        });
                    }
                reads_partitioned += n_reads;
            }
            w->flags.reset();
            std::vector<char*> text(parts, nullptr);
            std::vector<uint64_t> len(parts, 0);
            std::vector<int> rc(parts, MTSV_OK);
            std::vector<std::string> msg(parts);
            auto fmt = [&](unsigned k) {
                if (out_fd < 0) return;  // (no results file: --matched / --unmatched alone)
                if (cli_records) {
                    if (w->read_first)
                        for (uint64_t i = cut[k]; i < cut[k + 1]; i++) record_read(w->assigns, i) -= w->read_first;
                    rc[k] = cli_assign_long ? mtsv_format_assignments_gi((const mtsv_assignment_gi*)(w->assigns + cut[k] * a_rec), cut[k + 1] - cut[k],
                                                                         w->rb->ids.data(), w->rb->id_off.data(), n_reads, &text[k], &len[k])
                                            : mtsv_format_assignments((const mtsv_assignment*)(w->assigns + cut[k] * a_rec), cut[k + 1] - cut[k],
                                                                      w->rb->ids.data(), w->rb->id_off.data(), n_reads, &text[k], &len[k]);
                    if (rc[k] != MTSV_OK) msg[k] = mtsv_last_error();  // thread-local
                    return;
                }
                if (w->read_first)
                    for (uint64_t i = cut[k]; i < cut[k + 1]; i++) w->hits[i].read -= w->read_first;
                rc[k] = mtsv_format_results(w->hits + cut[k], cut[k + 1] - cut[k], w->rb->ids.data(), w->rb->id_off.data(), n_reads,
                                            long_fmt, &text[k], &len[k]);
                if (rc[k] != MTSV_OK) msg[k] = mtsv_last_error();  // thread-local
            };
            if (parts > 1) {
                for (unsigned k = 1; k < parts; k++) fmt_pool.submit([&fmt, k] { fmt(k); });
                fmt(0);
                fmt_pool.wait_all();
            } else {
                fmt(0);
            }
            w->hits_owner.reset();  // (the array goes back to the library's pool with the last batch of its call)
            w->assigns_owner.reset();
            acc(t_fmt, now() - t_f0);
            bool ok = true;
            for (unsigned k = 0; k < parts; k++)
                if (rc[k] != MTSV_OK) {
                    if (ok) logmsg("ERROR", "Error running query: " + msg[k]);
                    set_code(2);
                    ok = false;
                }
            if (ok && !failed() && !write_failed.load() && out_fd >= 0) {
                for (unsigned k = 0; k < parts; k++) {
                    const off_t at = out_pos;
                    out_pos += (off_t)len[k];
                    char* tx = text[k];
                    const uint64_t ln = len[k];
                    text[k] = nullptr;  // the write job owns it now
                    write_pool.submit([tx, ln, at, out_fd, &write_failed, &set_code] {
                        uint64_t done = 0;
                        while (done < ln) {
                            ssize_t r = pwrite(out_fd, tx + done, ln - done, at + (off_t)done);
                            if (r <= 0) {
                                write_failed.store(true);
                                set_code(11);  // binner.rs:136-139: the producer and the workers stop at once
                                break;
                            }
                            done += (uint64_t)r;
                        }
                        mtsv_free(tx);
                    });
                }
            }
            for (unsigned k = 0; k < parts; k++) mtsv_free(text[k]);
            // at most about two batches of text wait for the disk: the file stays a prefix of the results up to the
            // writes in flight (resume reads its last line), and formatted text does not pile up behind a slow disk
            {
                const double t_a = now();
                write_pool.wait_below(2 * (size_t)host_threads + 1);
                acc(t_write_wait, now() - t_a);
            }
            pool.put(std::move(w->rb));
            if (!ok) continue;
            total += n_reads;
            logmsg("DEBUG", "taxonomic binning: " + std::to_string(total) + " reads done");
        }
        write_pool.wait_all();
        if (write_failed.load()) {
            logmsg("ERROR", "Error writing to result file");
            set_code(11);  // binner.rs:136-139
        }
    });

    auto gpu_worker = [&](size_t wk) {
        mtsv_batch* ws = chunked && !merged ? nullptr : ws_ready[wk];  // one index: this worker's own workspace on its device (--merge-on-gpu: its collector)
        for (;;) {
            const double t_p = now();
            std::vector<std::unique_ptr<Work>> group;
            if (chunked) {
                group.push_back(parsed.pop());
                if (!group[0]) break;
            } else {
                // a full group, or what there is when no call is running on any device (the start of the input, a slow parser)
                // (--filter-index: a call's reads must fit the chain's workspaces as one resident batch)
                group = parsed.pop_group(kGroupReads, group_max, [&] { return calls_in_flight.load() == 0; }, filtered ? chain_bases : ~0ull);
                if (group.empty()) break;
            }
            acc(t_gpu_wait, now() - t_p);
            if (failed()) continue;  // drain
            if (filtered && (group.size() == 1 && (group[0]->rb->bases.size() > chain_bases || group[0]->rb->n() > chain_reads))) {
                logmsg("ERROR", "Error running query: a batch of reads holds more than " + std::to_string(chain_bases) + " bases, which the workspaces behind a filter index were sized for: give a smaller --batch-reads");
                set_code(2);
                continue;
            }
            uint64_t group_reads = 0;
            for (auto& w : group) group_reads += w->rb->n();
            calls_in_flight++;
            struct InFlight {
                std::atomic<int>& c;
                ~InFlight() { c--; }
            } in_flight{calls_in_flight};
            const double t_g = now();
            int rc;
            mtsv_hit* hits = nullptr;
            uint64_t n_hits = 0;
            uint8_t* assigns = nullptr;  // records of a_rec bytes
            uint64_t n_assigns = 0;
            auto download_records = [&](mtsv_batch* from) {
                return cli_assign_long ? mtsv_batch_download_assignments_gi(from, (mtsv_assignment_gi**)&assigns, &n_assigns, nullptr)
                                       : mtsv_batch_download_assignments(from, (mtsv_assignment**)&assigns, &n_assigns, nullptr);
            };
            if (merged) {
                auto& w = group[0];
                if (w->rb->n() > merge_reads || w->rb->bases.size() > merge_bases) {
                    logmsg("ERROR", "Error running query: a batch of reads holds more than " + std::to_string(merge_reads) + " reads or " + std::to_string(merge_bases) +
                                        " bases, which the chunks' workspaces were sized for: give a smaller --batch-reads");
                    set_code(2);
                    continue;
                }
                // the reads go up once; the other chunks receive them in HBM; every chunk runs; the collector merges
                auto& cw = cws[wk];
                rc = mtsv_batch_upload(cw[0], w->rb->bases.data(), w->rb->off.data(), w->rb->n());
                for (size_t c = 1; c < cw.size() && rc == MTSV_OK; c++) rc = mtsv_batch_copy_reads(cw[c], cw[0], nullptr);
                for (size_t c = 0; c < cw.size() && rc == MTSV_OK; c++) rc = mtsv_batch_run(cw[c], &p);
                if (rc == MTSV_OK) rc = mtsv_batch_merge_runs(ws, cw.data(), (int)cw.size(), nullptr);
                if (rc == MTSV_OK) rc = cli_records ? download_records(ws) : mtsv_batch_download(ws, &hits, &n_hits);
            } else if (chunked) {
                auto& w = group[0];
                rc = mtsv_bin_batch_chunks(idx.data(), chunk_dev.data(), (int)idx.size(), w->rb->bases.data(), w->rb->off.data(), w->rb->n(), &p,
                                           &hits, &n_hits);
            } else {
                std::vector<const uint8_t*> pb;
                std::vector<const uint64_t*> po;
                std::vector<uint64_t> pn;
                for (auto& w : group) {
                    pb.push_back(w->rb->bases.data());
                    po.push_back(w->rb->off.data());
                    pn.push_back(w->rb->n());
                }
                rc = mtsv_batch_run_host_parts(filtered ? fws[wk][0] : ws, (int)group.size(), pb.data(), po.data(), pn.data(), &p);
                // the chain: what no filter matched goes down the stages and into the database's workspace, in HBM
                for (size_t k = 0; k < n_filters && rc == MTSV_OK; k++) {
                    mtsv_batch* next = k + 1 < n_filters ? fws[wk][k + 1] : ws;
                    uint64_t kept = 0, kept_bases = 0, n_in = k ? 0 : group_reads;
                    if (k) {
                        mtsv_batch_stats st;
                        rc = mtsv_batch_stats_get(fws[wk][k], &st);
                        n_in = st.n_reads;
                    }
                    if (rc == MTSV_OK) rc = mtsv_batch_take_reads(next, fws[wk][k], MTSV_KEEP_UNMATCHED, &kept, &kept_bases, nullptr);
                    if (rc == MTSV_OK) {
                        stage_in[k] += n_in;
                        stage_removed[k] += n_in - kept;
                        rc = mtsv_batch_run(next, &p);
                    }
                }
                if (rc == MTSV_OK && cli_records) rc = download_records(ws);
                else if (rc == MTSV_OK && match_mode != MTSV_MATCH_ONLY) rc = mtsv_batch_download(ws, &hits, &n_hits);  // (flags only: there are none)
            }
            std::shared_ptr<uint64_t> flags;
            if (rc == MTSV_OK && partition) {
                uint64_t *words = nullptr, n_flagged = 0, n_match = 0;
                rc = mtsv_batch_match_flags(ws, &words, &n_flagged, &n_match);
                if (rc == MTSV_OK) {
                    flags = std::shared_ptr<uint64_t>(words, [](uint64_t* q) { mtsv_free(q); });
                    reads_matched += n_match;
                    if (n_flagged != group_reads) {
                        logmsg("ERROR", "Error running query: match flags for " + std::to_string(n_flagged) + " reads, the call held " + std::to_string(group_reads));
                        set_code(2);
                        continue;
                    }
                }
            }
            if (rc != MTSV_OK) {
                logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
                set_code(2);
                continue;
            }
            acc(t_gpu, now() - t_g);
            if (cli_timing) {
                char what[96];
                snprintf(what, sizeof what, "worker %zu: call on %llu reads in %zu blocks took %.2f ms, ended", wk, (unsigned long long)group_reads,
                         group.size(), (now() - t_g) * 1e3);
                mark(what);
            }
            // every batch gets its slice of the hits, read numbers relative to the batch
            // (the boundaries by bisection, the renumbering on the formatting threads: a pass over a million hits between two
            //  calls was 1.7 ms of every 8 the worker spent per megaread)
            std::shared_ptr<void> owner(hits, [](void* q) { mtsv_hits_free((mtsv_hit*)q); });
            std::shared_ptr<void> a_owner(assigns, [](void* q) { mtsv_free(q); });
            uint64_t first = 0, at = 0, a_at = 0;
            for (auto& w : group) {
                const uint64_t nr = w->rb->n();
                if (cli_records) {
                    uint64_t lo = a_at, hi = n_assigns;  // the first record of a later batch
                    while (lo < hi) {
                        const uint64_t mid = lo + (hi - lo) / 2;
                        if (record_read(assigns, mid) < first + nr) lo = mid + 1;
                        else hi = mid;
                    }
                    const uint64_t a_end = lo;
                    w->assigns = assigns + a_at * a_rec;
                    w->n_assigns = a_end - a_at;
                    w->assigns_owner = a_owner;
                    a_at = a_end;
                }
                const uint64_t end = (uint64_t)(std::partition_point(hits + at, hits + n_hits, [&](const mtsv_hit& h) { return h.read < first + nr; }) - hits);
                w->hits = hits + at;
                w->n_hits = end - at;
                w->read_first = first;
                w->hits_owner = owner;
                w->flags = flags;
                at = end;
                first += nr;
            }
            for (auto& w : group) done.push(std::move(w));
        }
        mark("worker out of batches");
    };
    {
        std::vector<std::thread> workers;
        for (size_t wk = 1; wk < n_workers; wk++) workers.emplace_back(gpu_worker, wk);
        gpu_worker(0);
        for (auto& t : workers) t.join();
    }
    done.close();
    writer.join();
    mark("writer done");
    // (the reader has handed on its last batch, or failed and said so, before the workers and the writer can end; what it
    //  may still be doing is closing its input -- unmapping 10 GB takes 45 ms -- and that is not part of the queries)
    struct ReaderJoin {
        std::thread& t;
        ~ReaderJoin() { t.join(); }
    } reader_join{reader};
    if (exit_code) return exit_code;
    if (out_fd >= 0 && ::close(out_fd) != 0) {
        logmsg("ERROR", "Error writing to result file");
        return 11;
    }
    mark("results file closed");
    for (int k = 0; k < 2; k++)
        if (part_fd[k] >= 0 && ::close(part_fd[k]) != 0) {
            logmsg("ERROR", std::string("Error writing to ") + (k ? a.unmatched : a.matched));
            return 11;
        }
    if (partition)
        logmsg("INFO", "Partitioned " + std::to_string(reads_partitioned.load()) + " reads: " + std::to_string(reads_matched.load()) + " matched, " +
                           std::to_string(reads_partitioned.load() - reads_matched.load()) + " unmatched.");
    for (size_t k = 0; k < n_filters; k++)
        logmsg("INFO", "Filter stage " + std::to_string(k + 1) + " (" + filter_paths[k] + "): removed " + std::to_string(stage_removed[k].load()) + " of " +
                           std::to_string(stage_in[k].load()) + " reads.");
    if (!a.report.empty()) {
        // the workers' counts add up: every read went through exactly one of their workspaces
        mtsv_taxon_stats* sum = nullptr;
        uint64_t n_sum = 0, total_reads = 0;
        bool ok = true;
        for (auto* ws : ws_ready) {
            mtsv_taxon_stats *rows = nullptr, *merged = nullptr;
            uint64_t n_rows = 0, n_merged = 0, reads = 0;
            ok = ok && mtsv_batch_taxa_report(ws, &rows, &n_rows, &reads, nullptr, 0) == MTSV_OK &&
                 mtsv_merge_taxa_reports(sum, n_sum, rows, n_rows, &merged, &n_merged) == MTSV_OK;
            mtsv_free(rows);
            if (!ok) break;
            mtsv_free(sum);
            sum = merged;
            n_sum = n_merged;
            total_reads += reads;
        }
        char* text = nullptr;
        uint64_t text_len = 0;
        if (!ok || mtsv_format_taxa_report(sum, n_sum, total_reads, &text, &text_len) != MTSV_OK) {
            logmsg("ERROR", std::string("Error running query: ") + mtsv_last_error());
            return 2;
        }
        FILE* rf = fopen(a.report.c_str(), "wb");
        const bool written = rf && fwrite(text, 1, text_len, rf) == text_len;
        if ((rf && fclose(rf) != 0) || !written) {
            logmsg("ERROR", "Error writing to taxa report file");
            return 11;
        }
        mtsv_free(text);
        mtsv_free(sum);
        mark("taxa report written");
    }
    struct timespec w1;
    clock_gettime(CLOCK_MONOTONIC, &w1);
    char msg[160];
    snprintf(msg, sizeof msg, "All worker and result consumer threads terminated. Took %.3f seconds.",
             (w1.tv_sec - w0.tv_sec) + (w1.tv_nsec - w0.tv_nsec) * 1e-9);
    logmsg("INFO", msg);
    if (cli_timing)
        fprintf(stderr, "[cli timing] batches %llu; reader: producing %.3f s, queue full %.3f s; gpu workers: in the library %.3f s, waiting for batches %.3f s; "
                        "writer: formatting %.3f s, waiting for hits %.3f s, waiting for the disk %.3f s\n",
                (unsigned long long)n_batches, t_ingest_wait.load() * 1e-6, t_push_wait.load() * 1e-6, t_gpu.load() * 1e-6, t_gpu_wait.load() * 1e-6,
                t_fmt.load() * 1e-6, t_done_wait.load() * 1e-6, t_write_wait.load() * 1e-6);
    if (cli_timing && getenv("MTSV_CLI_MARKS"))
        for (auto& m : marks) fprintf(stderr, "[cli timing] %9.3f ms  %s\n", m.second * 1e3, m.first.c_str());
    setup_mark("queries done");
    // The results are on their way to the disk (close() has returned) and the log line is out: leave.  Handing 2 GB of
    // page-locked blocks, the workspaces and the resident index back piece by piece takes 0.3 s that the kernel's own
    // teardown of the process does not need (MTSV_CLI_CLEAN_EXIT=1: free everything, for leak checkers).
    if (!getenv("MTSV_CLI_CLEAN_EXIT")) {
        fflush(nullptr);  // (the reader thread may still be unmapping its input: it ends with the process)
        _exit(0);
    }
    for (auto* ws : ws_ready) mtsv_batch_free(ws);  // (30 ms per workspace: after the queries' clock, like the index)
    for (auto& stage : fws)
        for (auto* ws : stage) mtsv_batch_free(ws);
    for (auto& chunk_ws : cws)
        for (auto* ws : chunk_ws) mtsv_batch_free(ws);
    setup_mark("workspaces freed");
    for (auto* ix : idx) mtsv_index_free(ix);
    for (auto* ix : fidx) mtsv_index_free(ix);
    setup_mark("index freed");
    return 0;
}
