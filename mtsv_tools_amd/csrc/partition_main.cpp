// mtsv-partition -- split a read file into the reads whose ID occurs in mtsv results files and the reads whose ID
// does not (the reference's tool of the same name, src/bin/mtsv-partition.rs): host, rRNA or contaminant depletion
// before the real binning, or pulling out the unassigned reads after it.  Host only: no HIP, no libmtsv_amd.
//
//   mtsv-partition --results R1 [R2 ..] (--fasta F | --fastq F) --matched M --unmatched U [-v]
//
// Results files (:34-54) are plain text: lines that are empty after trimming are skipped, the read ID is everything
// before the LAST ':' of a line; a line without ':' or with an empty ID ends the tool with exit 2.  The reads file
// may be gzip-compressed (magic sniff, :20-32); a record's ID is the first token of its header, split at space or
// tab, as in mtsv-binner.  A record goes to --matched when its ID is in the set and to --unmatched otherwise, in
// input order, in the record format of fastx_ingest.hpp's write_record.  A read or write failure is exit 3, a usage
// error exit 1.  Two records with the same ID share a fate here; mtsv-binner --matched / --unmatched, which decides
// on the GPU without a results file, takes every read by itself.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "cli_common.hpp"
#include "fastx_ingest.hpp"

namespace {

void logmsg(const char* level, const std::string& msg) { mtsv_cli::logmsg("mtsv_partition", level, msg); }

[[noreturn]] void usage_error(const std::string& m) {
    fprintf(stderr,
            "error: %s\n\nUSAGE:\n    mtsv-partition [FLAGS] --results <RESULTS>... --matched <MATCHED> --unmatched <UNMATCHED> <--fasta <FASTA>|--fastq <FASTQ>>\n",
            m.c_str());
    exit(1);  // clap usage errors
}

bool blank(const std::string& l) { return l.find_first_not_of(" \t\r\n\v\f") == std::string::npos; }

// read_ids_from_results: "" on success, else the error text
std::string read_ids(const std::vector<std::string>& paths, std::unordered_set<std::string>& ids) {
    for (const std::string& path : paths) {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) return path + ": " + strerror(errno);
        std::string line;
        char buf[1 << 16];
        auto take = [&](std::string& l) -> bool {
            if (!l.empty() && l.back() == '\r') l.pop_back();  // (lines end with "\n" or "\r\n")
            if (!blank(l)) {
                const size_t c = l.rfind(':');
                if (c == std::string::npos || c == 0) return false;
                ids.insert(l.substr(0, c));
            }
            return true;
        };
        size_t got;
        bool ok = true;
        while (ok && (got = fread(buf, 1, sizeof buf, f)) > 0) {
            size_t at = 0;
            while (ok && at < got) {
                const char* nl = (const char*)memchr(buf + at, '\n', got - at);
                if (!nl) {
                    line.append(buf + at, got - at);
                    break;
                }
                line.append(buf + at, (size_t)(nl - (buf + at)));
                at = (size_t)(nl - buf) + 1;
                ok = take(line);
                if (ok) line.clear();
            }
        }
        const bool io_error = ferror(f) != 0;
        fclose(f);
        if (io_error) return path + ": read error";
        if (ok && !line.empty()) ok = take(line);
        if (!ok) return "InvalidHeader(" + line + ")";
    }
    return std::string();
}

struct Out {
    FILE* f = nullptr;
    std::string buf;
    bool flush() {
        const bool ok = buf.empty() || fwrite(buf.data(), 1, buf.size(), f) == buf.size();
        buf.clear();
        return ok;
    }
};

}  // namespace

int main(int argc, char** argv) {
    std::vector<std::string> results;
    std::string fasta, fastq, matched, unmatched;
    for (int i = 1; i < argc; i++) {
        std::string k = argv[i];
        std::string inline_val;
        bool has_inline = false;
        const size_t eq = k.find('=');
        if (k.rfind("--", 0) == 0 && eq != std::string::npos) {
            inline_val = k.substr(eq + 1);
            k = k.substr(0, eq);
            has_inline = true;
        }
        auto val = [&]() -> std::string {
            if (has_inline) return inline_val;
            if (i + 1 >= argc) usage_error("The argument '" + k + "' requires a value but none was supplied");
            return argv[++i];
        };
        if (k == "--results") {
            results.push_back(val());
            while (!has_inline && i + 1 < argc && argv[i + 1][0] != '-') results.push_back(argv[++i]);  // --results R1 R2 ..
        } else if (k == "--fasta") fasta = val();
        else if (k == "--fastq") fastq = val();
        else if (k == "--matched") matched = val();
        else if (k == "--unmatched") unmatched = val();
        else if (k == "-v") mtsv_cli::verbose() = true;
        else if (k == "-h" || k == "--help") {
            printf("mtsv-partition -- split reads into matched / unmatched sets based on mtsv results\n"
                   "    --results R1 [R2 ..]   mtsv results files (the read ID is what stands before the last ':' of a line)\n"
                   "    --fasta F | --fastq F  the reads (plain or gzip)\n"
                   "    --matched M            output: the records whose ID occurs in the results\n"
                   "    --unmatched U          output: the others\n"
                   "    -v                     debug-level logging\n"
                   "Records that share an ID share a fate.  mtsv-binner --matched / --unmatched makes the same split while it bins.\n");
            return 0;
        } else if (k == "-V" || k == "--version") {
            printf("mtsv-partition 2.1.0 (mtsv_tools_amd)\n");
            return 0;
        } else
            usage_error("Found argument '" + k + "' which wasn't expected, or isn't valid in this context");
    }
    if (results.empty()) usage_error("The following required arguments were not provided: --results <RESULTS>...");
    if (fasta.empty() == fastq.empty())
        usage_error(fasta.empty() ? "The following required arguments were not provided: --fasta <FASTA> | --fastq <FASTQ>"
                                  : "The argument '--fasta <FASTA>' cannot be used with '--fastq <FASTQ>'");
    if (matched.empty()) usage_error("The following required arguments were not provided: --matched <MATCHED>");
    if (unmatched.empty()) usage_error("The following required arguments were not provided: --unmatched <UNMATCHED>");

    std::unordered_set<std::string> ids;
    const std::string why = read_ids(results, ids);
    if (!why.empty()) {
        logmsg("ERROR", "Unable to parse results: " + why);
        return 2;
    }
    logmsg("DEBUG", std::to_string(ids.size()) + " read IDs in the results");

    const bool is_fastq = fasta.empty();
    const std::string input = is_fastq ? fastq : fasta;
    mtsv_ingest::keep_records() = true;
    mtsv_ingest::FastxReader rd;
    rd.fastq = is_fastq;
    auto fail = [](const std::string& m) {
        logmsg("ERROR", "Error partitioning reads: " + m);
        return 3;
    };
    {
        FILE* probe = fopen(input.c_str(), "rb");  // (zlib's own message does not say why)
        if (!probe) return fail(input + ": " + strerror(errno));
        fclose(probe);
    }
    if (!rd.in.open(input)) return fail("cannot open " + input);
    Out out[2];
    out[0].f = fopen(matched.c_str(), "wb");
    if (!out[0].f) return fail(matched + ": " + strerror(errno));
    out[1].f = fopen(unmatched.c_str(), "wb");
    if (!out[1].f) return fail(unmatched + ": " + strerror(errno));
    mtsv_ingest::Record r;
    uint64_t n[2] = {0, 0};
    while (rd.next(r)) {
        const int side = ids.count(r.id) ? 0 : 1;
        mtsv_ingest::write_record(out[side].buf, is_fastq, r.id.data(), r.id.size(), r.desc.data(), r.desc.size(), r.seq.data(), r.seq.size(),
                                  r.qual.data());
        n[side]++;
        if (out[side].buf.size() >= (1u << 20) && !out[side].flush()) return fail("write error");
    }
    if (rd.error) return fail(rd.err_msg);
    for (auto& o : out)
        if (!o.flush() || fclose(o.f) != 0) return fail("write error");
    logmsg("DEBUG", std::to_string(n[0]) + " records matched, " + std::to_string(n[1]) + " unmatched");
    return 0;
}
