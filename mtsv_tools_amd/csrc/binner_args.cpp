// binner_args.cpp -- mtsv-binner's flags and their validation (mtsv-binner.rs:26-113, :140-262) and the resume rule (:347-411).
#include "binner_args.hpp"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <unordered_set>

#include "binner_handles.hpp"
#include "fastx_ingest.hpp"

namespace mtsv_cli {

[[noreturn]] void usage_error(const std::string& m) {
    fprintf(stderr, "error: %s\n\nUSAGE:\n    mtsv-binner [FLAGS] [OPTIONS] --index <INDEX> <--fasta <FASTA>|--fastq <FASTQ>>\n", m.c_str());
    exit(1);  // clap usage errors
}

namespace {

[[noreturn]] void refuse(const std::string& m) {  // a combination this command line rules out itself: no usage text
    fprintf(stderr, "error: %s\n", m.c_str());
    exit(1);
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
// a number of reads in 1..max, or the usage error of `flag`
uint64_t parse_reads(const std::string& v, const char* flag, unsigned long long max) {
    char* e = nullptr;
    errno = 0;
    const unsigned long long n = strtoull(v.c_str(), &e, 10);
    if (v.empty() || v[0] == '-' || *e || errno || n < 1 || n > max)
        usage_error(std::string("Invalid value for '") + flag + " <N>': a number of reads between 1 and " + std::to_string(max) + " is expected");
    return n;
}

void print_help() {
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
           "and --matched / --unmatched are derived; every read keeps its own ID and every file is the same),\n"
           "--interleaved [--pair-mode both|either|proper] [--max-insert N] [--unpaired-penalty N] (only with --fold-on-gpu:\n"
           "paired-end reads.  The input is one FASTA/FASTQ file whose records alternate mate 1 and mate 2; the reads are binned\n"
           "and folded as always, and after the last chunk the two mates' records are joined on the GPU into one line per pair,\n"
           "PAIR_ID:TAXID=EDIT,..., PAIR_ID the mates' common ID or their common stem when the IDs end in /1 and /2.  proper (the\n"
           "default): a TaxID is kept when both mates hit the same GI of it within --max-insert bases (default 1000) of each\n"
           "other, with the smallest sum of the two edits; the mates' orientation is not checked.  both: when both mates hit the\n"
           "TaxID, the sum of their smallest edits.  either: every TaxID either mate hit; one that only one mate hit carries that\n"
           "mate's edit plus --unpaired-penalty, which must be given.  --report counts pairs.  An odd number of records, or mates\n"
           "whose IDs do not agree, is an input error.  Not with --output-format long, --matched / --unmatched or an odd\n"
           "--read-offset; a run that would resume an existing results file is refused),\n"
           "--coverage TSV [--coverage-slack N|all] (only with --fold-on-gpu, and with records that carry GI and offset:\n"
           "--output-format long, or --interleaved --pair-mode proper.  Per reference sequence (TaxID, GI) the reads and alignments\n"
           "it took, the bases they span and the bases at least one of them covers, counted on the GPU from the accumulated\n"
           "records in a bitmap of one bit per reference base: columns taxid, gi, length, reads, alignments, aligned_bases, depth,\n"
           "covered_bases, breadth_pct, one line per reference with an alignment and one per TaxID (gi *) over all its\n"
           "references.  An alignment counts when its edit distance is within --coverage-slack (default 0) of its read's\n"
           "smallest; all: every alignment.  It spans the read's length from the start of its accepted window, which lies up\n"
           "to the edit tolerance before the match.  With --dedup every copy of a read counts),\n"
           "--alignments FILE (only with --fold-on-gpu, not with --dedup: after every chunk's run over a batch of reads the hits\n"
           "it accepted are aligned on the GPU, and one line per hit is appended to FILE,\n"
           "READ_ID<TAB>TAXID<TAB>GI<TAB>+|-<TAB>START<TAB>END<TAB>EDIT<TAB>CIGAR: the strand, the half-open interval of the\n"
           "match inside the GI on the forward strand, and the edit script with = X I D, in reference order.  Lines come chunk\n"
           "by chunk, batch by batch; each stands for itself, so the file may be sorted.  Reads of up to 256 bases.  Every other\n"
           "output is what it is without the flag),\n"
           "--variants TSV [--variant-taxa T1,T2,..] [--variant-slack N|all] [--min-depth N] [--min-alt-reads N] [--min-alt-frac F]\n"
           "(only with --fold-on-gpu, not with --dedup: after every chunk's run over a batch of reads the hits it accepted are\n"
           "aligned on the GPU and their edit scripts added up per reference position, in one accumulator for the whole run; after\n"
           "the last read TSV gets a header and one line per variant site, taxid, gi, pos (0-based), ref, depth, match, A, C, G, T,\n"
           "N, del, ins: how many reads match the reference there, show another base, skip the position, or carry extra bases in\n"
           "front of it (ref `.`: behind the sequence's last base).  A hit counts when its edit distance is within\n"
           "--variant-slack (default 0) of its read's smallest in that chunk; all: every hit.  A position is listed when its depth\n"
           "is at least --min-depth (default 1) and a count other than match is at least --min-alt-reads (default 1) and at least\n"
           "--min-alt-frac (0 .. 1, default 0) of the depth: by default every position where any read disagrees.  --variant-taxa:\n"
           "only references of these TaxIDs are counted; the counters take 33 bytes of device memory per reference base of the\n"
           "chunks, so a large database needs the list.  With --alignments as well the hits are aligned twice.  Reads of up to 256\n"
           "bases.  Every other output is what it is without the flag),\n"
           "--consensus FASTA [--consensus-stats TSV] [--consensus-min-depth N] [--consensus-min-frac F] [--consensus-min-breadth F]\n"
           "[--consensus-fill n|ref] [--consensus-width N] (only with --fold-on-gpu, not with --dedup: the same accumulator as\n"
           "--variants -- one per run, shared when both are given, described by --variant-taxa and --variant-slack -- is called\n"
           "once, after the last read, on the GPU: FASTA gets a consensus sequence per reference with a covered position, headed\n"
           ">GI-TAXID as mtsv-build reads it, in lines of --consensus-width (default 60; 0: one line).  A position whose depth is\n"
           "below --consensus-min-depth (default 1), whose most frequent call is a read N or has less than --consensus-min-frac\n"
           "(0 .. 1, default 0.5) of the depth is written as N (--consensus-fill n, the default) or as the reference base in lower\n"
           "case (ref); otherwise the reference base, the substituted base, or nothing where most reads skip the position.\n"
           "Insertions cannot be spelled: the accumulator counts the reads that insert in front of a position, not their bases; they\n"
           "are only counted, as ins_sites.  A reference is left out when less than --consensus-min-breadth (0 .. 1, default 0) of\n"
           "it is covered.  --consensus-stats: a header and one line per written reference and per TaxID (gi *), taxid, gi, length,\n"
           "covered, breadth_pct, mean_depth, cons_len, ref, sub, del, low, ambiguous, ins_sites, identity_pct = ref / (ref + sub +\n"
           "del).  Every other output is what it is without the flag)\n");
}

// a number in 0 .. 2^32 - 1, or the usage error of `flag`
uint32_t parse_u32_flag(const std::string& v, const char* flag) {
    char* e = nullptr;
    errno = 0;
    const unsigned long long n = strtoull(v.c_str(), &e, 10);
    if (v.empty() || v[0] == '-' || *e || errno || n > 0xffffffffull)
        usage_error(std::string("Invalid value for '") + flag + " <N>': a number between 0 and 4294967295 is expected");
    return (uint32_t)n;
}

// --merge-on-gpu and --fold-on-gpu alike: a list of chunks, one device, and not --parse-only
void require_chunks_on_one_device(const Args& a, const char* flag, const char* on_that_device) {
    if (split_list(a.index, ',').size() < 2) refuse(std::string("'") + flag + "' needs a list of two or more index chunks ('--index a,b,..')");
    if (a.devices.size() != 1) refuse(std::string("'") + flag + "' needs exactly one '--devices' entry: " + on_that_device);
    if (a.parse_only) usage_error(std::string("The argument '--parse-only' cannot be used with '") + flag + "'");
}

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
    mtsv_ingest::FastxReader rd;
    rd.fastq = fastq;
    if (!rd.in.open(input)) return -1;
    mtsv_ingest::Record r;
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

// which flags go together: every violation is a usage error (exit 1), the first one in this order is the one reported
void check_combinations(const Args& a) {
    const bool chunk_list = a.index.find(',') != std::string::npos;
    const bool on_one_device = a.merge_gpu || a.fold_gpu;  // the chunks' hits are merged per read on the device
    const bool partition = !a.matched.empty() || !a.unmatched.empty();
    const bool filtered = !a.filter_index.empty();
    if (a.fasta.empty() == a.fastq.empty())
        usage_error(a.fasta.empty() ? "The following required arguments were not provided: --fasta <FASTA> | --fastq <FASTQ>"
                                    : "The argument '--fasta <FASTA>' cannot be used with '--fastq <FASTQ>'");
    if (a.index.empty() && !a.parse_only) usage_error("The following required arguments were not provided: --index <INDEX>");
    if (a.text_gpu) {
        if (a.merge_gpu && !a.fold_gpu) usage_error("The argument '--text-on-gpu' cannot be used with '--merge-on-gpu': it writes the lines of '--fold-on-gpu'");
        if (!a.fold_gpu) usage_error("The argument '--text-on-gpu' requires '--fold-on-gpu'");
    }
    if (a.fold_prefetch && !a.fold_gpu) usage_error("The argument '--fold-prefetch' requires '--fold-on-gpu'");
    if (a.dedup && !a.fold_gpu) usage_error("The argument '--dedup' requires '--fold-on-gpu'");
    if (!a.interleaved) {
        if (!a.pair_mode.empty()) usage_error("The argument '--pair-mode <MODE>' requires '--interleaved'");
        if (!a.max_insert.empty()) usage_error("The argument '--max-insert <N>' requires '--interleaved'");
        if (!a.unpaired_penalty.empty()) usage_error("The argument '--unpaired-penalty <N>' requires '--interleaved'");
    } else {
        if (!a.fold_gpu) usage_error("The argument '--interleaved' requires '--fold-on-gpu'");
        if (a.output_format == "long") usage_error("The argument '--interleaved' cannot be used with '--output-format long': a pair's line is PAIR_ID:TAXID=EDIT,...");
        if (partition) usage_error("The argument '--interleaved' cannot be used with '--matched <PATH>' / '--unmatched <PATH>'");
        if (filtered) usage_error("The argument '--interleaved' cannot be used with '--filter-index <INDEX>'");
        if (!a.pair_mode.empty() && a.pair_mode != "both" && a.pair_mode != "either" && a.pair_mode != "proper")
            usage_error("'" + a.pair_mode + "' isn't a valid value for '--pair-mode <MODE>' [possible values: both, either, proper]");
        if (a.pair_mode == "either" && a.unpaired_penalty.empty())
            usage_error("The argument '--pair-mode either' requires '--unpaired-penalty <N>': what a mate that did not align costs cannot be derived from the records");
    }
    if (a.coverage.empty()) {
        if (!a.coverage_slack.empty()) usage_error("The argument '--coverage-slack <N|all>' requires '--coverage <TSV>'");
    } else {
        if (!a.fold_gpu) usage_error("The argument '--coverage <TSV>' requires '--fold-on-gpu'");
        const bool proper = a.interleaved && (a.pair_mode.empty() || a.pair_mode == "proper");
        if (a.output_format != "long" && !proper)
            usage_error("The argument '--coverage <TSV>' needs records with GI and offset: give '--output-format long', or '--interleaved --pair-mode proper'");
    }
    if (!a.alignments.empty()) {
        if (!a.fold_gpu) refuse("'--alignments <FILE>' requires '--fold-on-gpu': the hits are aligned where a chunk's run leaves them, on the device");
        if (a.dedup) refuse("'--alignments <FILE>' cannot be used with '--dedup': only the representatives of identical reads are binned");
        if (a.alignments == a.results) refuse("'--alignments <FILE>' and '-m/--results <RESULTS>' name the same file");
    }
    if (a.variants.empty()) {
        // (--variant-taxa and --variant-slack describe the run's one pileup: --consensus makes one too)
        if (!a.variant_taxa.empty() && a.consensus.empty()) usage_error("The argument '--variant-taxa <T1,T2,..>' requires '--variants <TSV>'");
        if (!a.variant_slack.empty() && a.consensus.empty()) usage_error("The argument '--variant-slack <N|all>' requires '--variants <TSV>'");
        if (!a.min_depth.empty()) usage_error("The argument '--min-depth <N>' requires '--variants <TSV>'");
        if (!a.min_alt_reads.empty()) usage_error("The argument '--min-alt-reads <N>' requires '--variants <TSV>'");
        if (!a.min_alt_frac.empty()) usage_error("The argument '--min-alt-frac <F>' requires '--variants <TSV>'");
    } else {
        if (!a.fold_gpu) refuse("'--variants <TSV>' requires '--fold-on-gpu': the hits are aligned where a chunk's run leaves them, on the device");
        if (a.dedup) refuse("'--variants <TSV>' cannot be used with '--dedup': only the representatives of identical reads are binned");
        if (a.variants == a.results) refuse("'--variants <TSV>' and '-m/--results <RESULTS>' name the same file");
        if (a.variants == a.alignments) refuse("'--variants <TSV>' and '--alignments <FILE>' name the same file");
    }
    if (a.consensus.empty()) {
        const std::pair<const std::string*, const char*> sub[] = {{&a.consensus_stats, "--consensus-stats <TSV>"},   {&a.consensus_min_depth, "--consensus-min-depth <N>"},
                                                                  {&a.consensus_min_frac, "--consensus-min-frac <F>"}, {&a.consensus_min_breadth, "--consensus-min-breadth <F>"},
                                                                  {&a.consensus_fill, "--consensus-fill <n|ref>"},     {&a.consensus_width, "--consensus-width <N>"}};
        for (const auto& f : sub)
            if (!f.first->empty()) usage_error(std::string("The argument '") + f.second + "' requires '--consensus <FASTA>'");
    } else {
        if (!a.fold_gpu) refuse("'--consensus <FASTA>' requires '--fold-on-gpu': the hits are aligned where a chunk's run leaves them, on the device");
        if (a.dedup) refuse("'--consensus <FASTA>' cannot be used with '--dedup': only the representatives of identical reads are binned");
        // every consensus file against every other output file
        const std::pair<const std::string*, const char*> mine[] = {{&a.consensus, "--consensus <FASTA>"}, {&a.consensus_stats, "--consensus-stats <TSV>"}};
        const std::pair<const std::string*, const char*> others[] = {{&a.consensus, "--consensus <FASTA>"}, {&a.results, "-m/--results <RESULTS>"},
                                                                     {&a.alignments, "--alignments <FILE>"}, {&a.variants, "--variants <TSV>"},
                                                                     {&a.report, "--report <TSV>"},          {&a.coverage, "--coverage <TSV>"},
                                                                     {&a.matched, "--matched <PATH>"},       {&a.unmatched, "--unmatched <PATH>"}};
        for (const auto& m : mine)
            for (const auto& o : others)
                if (m.first != o.first && !m.first->empty() && *m.first == *o.first)
                    refuse(std::string("'") + m.second + "' and '" + o.second + "' name the same file");
    }
    if (a.merge_gpu) require_chunks_on_one_device(a, "--merge-on-gpu", "every chunk is made resident on that device");
    if (a.fold_gpu) {
        if (a.merge_gpu) usage_error("The argument '--merge-on-gpu' cannot be used with '--fold-on-gpu'");
        if (filtered) usage_error("The argument '--filter-index <INDEX>' cannot be used with '--fold-on-gpu'");
        require_chunks_on_one_device(a, "--fold-on-gpu", "the chunks take turns on that device");
    }
    // a read's taxa come from several chunks there and per-chunk counters do not add up
    if (!on_one_device && !a.report.empty() && chunk_list)
        refuse("'--report <TSV>' cannot be used with a list of index chunks ('--index a,b,..'): run mtsv-collapse --report on the results file instead, or give '--merge-on-gpu' (one device)");
    if (partition && a.parse_only) usage_error("The argument '--parse-only' cannot be used with '--matched <PATH>' / '--unmatched <PATH>'");
    // (the flags of the chunks would have to be OR-ed per read)
    if (!on_one_device && partition && chunk_list)
        refuse("'--matched <PATH>' / '--unmatched <PATH>' cannot be used with a list of index chunks ('--index a,b,..'): run mtsv-partition on the results file instead, or give '--merge-on-gpu' (one device)");
    if (filtered && partition) usage_error("The argument '--filter-index <INDEX>' cannot be used with '--matched <PATH>' / '--unmatched <PATH>'");
    if (filtered && a.parse_only) usage_error("The argument '--parse-only' cannot be used with '--filter-index <INDEX>'");
    // (every chunk would need the survivors, and its hits merged per read)
    if (filtered && chunk_list)
        refuse("'--filter-index <INDEX>' cannot be used with a list of index chunks ('--index a,b,..'): filter first with '--unmatched <PATH>', then bin the chunks");
    if (!on_one_device && partition && !a.report.empty() && a.results.empty())
        usage_error("The argument '--report <TSV>' requires '-m/--results <RESULTS>': the report is counted from gathered hits, and '--matched' / '--unmatched' without a results file gather none");
    if (a.output_format != "default" && a.output_format != "long")
        usage_error("'" + a.output_format + "' isn't a valid value for '--output-format <OUTPUT_FORMAT>'");
}

// the numbers of the command line: a bad one panics; the reference's INFO / WARN lines are logged on the way
void resolve_params(const Args& a, Run& run) {
    const uint64_t t_flag = parse_usize(a.threads, "Invalid number entered for number of threads!");
    run.host_threads = (unsigned)std::min<uint64_t>(std::max<uint64_t>(t_flag, 8), std::max(1u, std::thread::hardware_concurrency()));
    if (const char* e = getenv("MTSV_HOST_THREADS")) run.host_threads = (unsigned)std::max(1, atoi(e));
    mtsv_params& p = run.params;
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
    run.read_offset = parse_usize(a.read_offset, "Invalid read offset entered!");
    if (seed_size == 0 || seed_size > 0xffffffffull || seed_gap == 0 || seed_gap > 0xffffffffull)
        panic("seed size / interval out of range");  // the reference panics on a zero step (itertools)
    p.seed_size = (uint32_t)seed_size;
    p.seed_interval = (uint32_t)seed_gap;
}

// the results path: none at all (exit 3), one that exists and is overwritten, refused (1) or resumed (scan failed: 4)
void resolve_results(const Args& a, Run& run) {
    if (a.results.empty() && !a.parse_only && !run.partition) {
        logmsg("ERROR", "No results path provided!");
        exit(3);
    }
    FILE* probe = run.have_results() ? fopen(a.results.c_str(), "rb") : nullptr;
    const bool exists = probe != nullptr;
    if (probe) fclose(probe);
    run.append = !a.force && exists;
    uint64_t resume = 0;
    if (a.force) {
        logmsg("INFO", "Forcing overwrite of " + a.results);
    } else if (exists && run.interleaved) {
        // (the resume scan looks for read IDs in the results file, and this one holds pair IDs)
        refuse("results file " + a.results + " exists and the run would resume it; '--interleaved' does not resume (its lines carry pair IDs, not read IDs): give --force-overwrite or another results path");
    } else if (exists && run.partition) {
        // a resumed run sees only the reads after the last one in the results file: the partition files would be incomplete
        refuse("results file " + a.results + " exists and the run would resume it; '--matched' / '--unmatched' need the whole input: give --force-overwrite or another results path");
    } else if (exists && run.folded()) {
        // (the accumulators hold a super-batch of the whole input's numbering; a resumed run is not what this path is for)
        refuse("results file " + a.results + " exists and the run would resume it; '--fold-on-gpu' does not resume: give --force-overwrite or another results path");
    } else if (exists && !a.parse_only) {
        logmsg("INFO", "Existing results detected at " + a.results + "; resuming previous run.");
        if (resume_offset(a.results, run.input, run.fastq, &resume) != 0) {
            logmsg("ERROR", "Error computing resume offset");
            exit(4);
        }
        logmsg("INFO", "Resuming after read offset " + std::to_string(resume) + " from " + a.results);
    }
    run.read_offset += resume;
}

}  // namespace

Args parse_args(int argc, char** argv) {
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
            for (const std::string& tok : split_list(val(), ',', true)) {
                char* e = nullptr;
                const long d = strtol(tok.c_str(), &e, 10);
                if (tok.empty() || *e || d < 0 || d > 1023) usage_error("Invalid value for '" + key + "': a comma-separated list of GPU ordinals is expected");
                a.devices.push_back((int)d);
            }
        } else if (key == "--batch-reads") a.batch_reads = parse_reads(val(), "--batch-reads", 0x7fffffffull);
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
        else if (key == "--interleaved") a.interleaved = true;
        else if (key == "--pair-mode") a.pair_mode = val();
        else if (key == "--max-insert") a.max_insert = val();
        else if (key == "--unpaired-penalty") a.unpaired_penalty = val();
        else if (key == "--coverage") a.coverage = val();
        else if (key == "--coverage-slack") a.coverage_slack = val();
        else if (key == "--alignments") a.alignments = val();
        else if (key == "--variants") a.variants = val();
        else if (key == "--variant-taxa") a.variant_taxa = val();
        else if (key == "--variant-slack") a.variant_slack = val();
        else if (key == "--min-depth") a.min_depth = val();
        else if (key == "--min-alt-reads") a.min_alt_reads = val();
        else if (key == "--min-alt-frac") a.min_alt_frac = val();
        else if (key == "--consensus") a.consensus = val();
        else if (key == "--consensus-stats") a.consensus_stats = val();
        else if (key == "--consensus-min-depth") a.consensus_min_depth = val();
        else if (key == "--consensus-min-frac") a.consensus_min_frac = val();
        else if (key == "--consensus-min-breadth") a.consensus_min_breadth = val();
        else if (key == "--consensus-fill") a.consensus_fill = val();
        else if (key == "--consensus-width") a.consensus_width = val();
        else if (key == "--fold-reads") a.fold_reads = parse_reads(val(), "--fold-reads", 0xffffffffull);
        else if (key == "-h" || key == "--help") {
            print_help();
            exit(0);
        } else if (key == "-V" || key == "--version") {
            printf("mtsv 2.1.0 (%s)\n", mtsv_version());
            exit(0);
        } else
            usage_error("Found argument '" + k + "' which wasn't expected, or isn't valid in this context");
    }
    return a;
}

Run resolve(const Args& a) {
    check_combinations(a);
    verbose() = a.verbose;
    Run run;
    run.fastq = a.fasta.empty();
    run.input = run.fastq ? a.fastq : a.fasta;
    run.results = a.results;
    run.report = a.report;
    run.part_path[0] = a.matched;
    run.part_path[1] = a.unmatched;
    run.index_paths = split_list(a.index, ',');
    run.filter_paths = split_list(a.filter_index, ',');
    run.devices = a.devices;
    run.mode = a.fold_gpu ? Mode::folded : a.merge_gpu ? Mode::merged : run.chunked() ? Mode::chunks : a.devices.size() > 1 ? Mode::replicated : Mode::single;
    run.partition = !a.matched.empty() || !a.unmatched.empty();
    run.filtered = !a.filter_index.empty();
    run.parse_only = a.parse_only;
    run.text_gpu = a.text_gpu;
    run.fold_prefetch = a.fold_prefetch;
    run.dedup = a.dedup;
    run.batch_reads = a.batch_reads;
    run.fold_reads = a.fold_reads;
    run.long_fmt = a.output_format == "long";
    run.interleaved = a.interleaved;
    if (a.interleaved) {
        run.pair_mode = a.pair_mode == "both" ? MTSV_PAIR_BOTH : a.pair_mode == "either" ? MTSV_PAIR_EITHER : MTSV_PAIR_PROPER;
        if (!a.max_insert.empty()) run.max_insert = parse_u32_flag(a.max_insert, "--max-insert");
        if (!a.unpaired_penalty.empty()) run.unpaired_penalty = parse_u32_flag(a.unpaired_penalty, "--unpaired-penalty");
        if (run.pair_mode == MTSV_PAIR_EITHER && run.unpaired_penalty >= 0x80000000u)
            usage_error("Invalid value for '--unpaired-penalty <N>': a number below 2147483648 is expected");
    }
    run.coverage = a.coverage;
    run.alignments = a.alignments;
    if (!a.coverage_slack.empty()) run.coverage_slack = a.coverage_slack == "all" ? 0xffffffffu : parse_u32_flag(a.coverage_slack, "--coverage-slack");
    run.variants = a.variants;
    if (!a.variant_taxa.empty())
        for (const std::string& tok : split_list(a.variant_taxa, ',', true)) {
            char* e = nullptr;
            errno = 0;
            const unsigned long long t = strtoull(tok.c_str(), &e, 10);
            if (tok.empty() || tok[0] == '-' || *e || errno || t > 0xffffffffull)
                usage_error("Invalid value for '--variant-taxa <T1,T2,..>': a comma-separated list of TaxIDs is expected");
            run.variant_taxa.push_back((uint32_t)t);
        }
    if (!a.variant_slack.empty()) run.variant_slack = a.variant_slack == "all" ? 0xffffffffu : parse_u32_flag(a.variant_slack, "--variant-slack");
    if (!a.min_depth.empty()) run.min_depth = parse_u32_flag(a.min_depth, "--min-depth");
    if (!a.min_alt_reads.empty()) run.min_alt_reads = parse_u32_flag(a.min_alt_reads, "--min-alt-reads");
    // a fraction as parts per million, rounded
    auto parse_ppm = [](const std::string& v, const char* flag) {
        char* e = nullptr;
        const double f = strtod(v.c_str(), &e);
        if (*e || e == v.c_str() || !(f >= 0.0 && f <= 1.0)) usage_error(std::string("Invalid value for '") + flag + " <F>': a fraction between 0 and 1 is expected");
        return (uint32_t)llround(f * 1e6);
    };
    if (!a.min_alt_frac.empty()) run.min_alt_ppm = parse_ppm(a.min_alt_frac, "--min-alt-frac");
    run.consensus = a.consensus;
    run.consensus_stats = a.consensus_stats;
    if (!a.consensus_min_depth.empty()) run.cons_min_depth = parse_u32_flag(a.consensus_min_depth, "--consensus-min-depth");
    if (!a.consensus_min_frac.empty()) run.cons_min_frac_ppm = parse_ppm(a.consensus_min_frac, "--consensus-min-frac");
    if (!a.consensus_min_breadth.empty()) run.cons_min_breadth_ppm = parse_ppm(a.consensus_min_breadth, "--consensus-min-breadth");
    if (!a.consensus_width.empty()) run.cons_width = parse_u32_flag(a.consensus_width, "--consensus-width");
    if (!a.consensus_fill.empty()) {
        if (a.consensus_fill != "n" && a.consensus_fill != "ref") usage_error("Invalid value for '--consensus-fill <n|ref>': 'n' or 'ref' is expected");
        run.cons_fill = a.consensus_fill == "ref" ? 1u : 0u;
    }
    resolve_params(a, run);
    if (run.interleaved && (run.read_offset & 1)) refuse("'--interleaved' needs an even '--read-offset': the reads are skipped pair by pair");
    resolve_results(a, run);
    return run;
}

void require_index_paths(const Run& run) {
    if (run.index_paths.empty()) usage_error("The following required arguments were not provided: --index <INDEX>");
    if (run.filtered && run.filter_paths.empty()) usage_error("The argument '--filter-index <INDEX>' requires a value but none was supplied");
}

}  // namespace mtsv_cli
