// parse.hip -- mtsv_fold_add_text (include/mtsv_amd.h): the hit parts of result lines go up as text, k_parse.hip makes the
// sorted, reduced record list of them in the fold's incoming array, and the fold takes it as it takes a run's list.  No
// record crosses to the host or comes from it; what comes down is counters and the records' TaxIDs, four bytes each, for the
// union the report's rows come from.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "fold.hpp"
#include "parse.hpp"

namespace mtsv {

TextParser::TextParser(int device_, hipStream_t stream_) : device(device_), stream(stream_) {
    trace = getenv("MTSV_TRACE") != nullptr;
    timing = getenv("MTSV_PARSE_TIMING") != nullptr;
    HIP_CHECK(hipSetDevice(device));
    ev.create();
}

TextParser::~TextParser() {
    if (hipSetDevice(device) != hipSuccess) (void)hipGetLastError();
    if (stream) (void)hipStreamSynchronize(stream);
}

void Fold::add_text(const char* hits, const uint64_t* line_off, const uint32_t* line_read, uint64_t n_lines, uint64_t* n_tokens, uint64_t* n_records,
                    float* device_ms) {
    if (n_tokens) *n_tokens = 0;
    if (n_records) *n_records = 0;
    if (device_ms) *device_ms = 0;
    if (n_lines) {
        if (line_off[0] != 0) throw std::runtime_error("arg: line 0: line_off[0] is " + std::to_string(line_off[0]) + ", not 0");
        for (uint64_t j = 0; j < n_lines; j++)
            if (line_off[j + 1] < line_off[j])
                throw std::runtime_error("arg: line " + std::to_string(j) + ": line_off descends from " + std::to_string(line_off[j]) + " to " +
                                         std::to_string(line_off[j + 1]));
    }
    const uint64_t N = n_lines ? line_off[n_lines] : 0;
    std::vector<uint32_t> taxa_in;
    if (!N) {  // (no line, or empty ones only: nothing is uploaded or launched)
        fold_in(0, taxa_in, nullptr);
        return;
    }
    HIP_CHECK(hipSetDevice(device));
    if (!parser) {
        parser.reset(new TextParser(device, stream));
        parser->tile = parse_tile;  // (read when the fold was created)
    }
    TextParser& P = *parser;
    if (N / P.tile >= 0xfffffff0ull) throw std::runtime_error("limit: " + std::to_string(N) + " bytes of text in tiles of " + std::to_string(P.tile));
    const uint32_t tiles = parse_tiles(N, P.tile);
    // ---- the text goes up; the tokens are counted ----
    const double t0 = P.timing ? now_ms() : 0;
    P.d_hits.room(stream, N + 16, "the text");
    P.d_line_off.room(stream, n_lines + 1, "the lines' offsets");
    P.d_line_read.room(stream, n_lines, "the lines' reads");
    P.d_tile_cnt.room(stream, tiles, "the tiles' tokens");
    P.d_tile_off.room(stream, (uint64_t)tiles + 1, "the tiles' offsets");
    P.d_sums.room(stream, (uint64_t)scan_tiles(tiles) + 1, "the scan's sums");
    P.d_ctr.room(stream, kParseCounters + 2, "the counters");
    uint64_t ctr[kParseCounters + 2];
    for (uint32_t k = 0; k < kParseCounters; k++) ctr[k] = k & 1 ? ~0ull : 0;
    ctr[kParseCounters] = ctr[kParseCounters + 1] = 0;
    HIP_CHECK(hipMemcpyAsync(P.d_hits.p, hits, N, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(P.d_line_off.p, line_off, (n_lines + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(P.d_line_read.p, line_read, n_lines * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(P.d_ctr.p, ctr, sizeof ctr, hipMemcpyHostToDevice, stream));
    if (P.timing) HIP_CHECK(hipStreamSynchronize(stream));
    const double t1 = P.timing ? now_ms() : 0;
    uint64_t* d_n_tok = P.d_ctr.p + kParseCounters;
    uint64_t* d_n_rec = d_n_tok + 1;
    HIP_CHECK(hipEventRecord(P.ev[0], stream));
    launch_parse_count(stream, P.d_hits.p, N, P.d_line_off.p, n_lines, P.tile, P.d_tile_cnt.p);
    launch_scan(stream, P.d_tile_cnt.p, tiles, P.d_sums.p, d_n_tok, P.d_tile_off.p);
    HIP_CHECK(hipEventRecord(P.ev[1], stream));
    uint64_t n_tok = 0;
    HIP_CHECK(hipMemcpyAsync(&n_tok, d_n_tok, sizeof n_tok, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (n_tokens) *n_tokens = n_tok;
    if (n_tok >= (1ull << 32)) throw std::runtime_error("limit: " + std::to_string(n_tok) + " tokens in one call, 2^32 or more");
    if (!n_tok) throw std::runtime_error("internal: " + std::to_string(N) + " bytes of text hold no token");
    // ---- the tokens are parsed and their runs found; whatever is refused is refused here, with the fold untouched ----
    P.d_raw_key.room(stream, n_tok * 16, "the raw tokens");
    P.d_raw_val.room(stream, n_tok * 16, "the raw tokens");
    P.d_flag.room(stream, n_tok, "the tokens' flags");
    P.d_place.room(stream, n_tok + 1, "the tokens' places");
    P.d_sums.room(stream, (uint64_t)scan_tiles((uint32_t)n_tok) + 1, "the scan's sums");
    HIP_CHECK(hipEventRecord(P.ev[2], stream));
    launch_parse_tokens(stream, grain, P.d_hits.p, N, P.d_line_off.p, P.d_line_read.p, n_lines, P.tile, P.d_tile_off.p, (uint32_t)n_tok, P.d_raw_key.p, P.d_raw_val.p,
                        P.d_ctr.p);
    launch_parse_heads(stream, grain, P.d_raw_key.p, P.d_raw_val.p, (uint32_t)n_tok, n_reads, P.d_flag.p, P.d_ctr.p);
    launch_scan(stream, P.d_flag.p, (uint32_t)n_tok, P.d_sums.p, d_n_rec, P.d_place.p);
    HIP_CHECK(hipEventRecord(P.ev[3], stream));
    HIP_CHECK(hipMemcpyAsync(ctr, P.d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    if (ctr[kParseCtrFormat])
        throw std::runtime_error("format: line " + std::to_string(ctr[kParseCtrFormat + 1]) + ": a token that is not " +
                                 (grain == MTSV_GRAIN_TAXID ? "TAXID=EDIT, TAXID-GI=EDIT or TAXID-GI-OFFSET=EDIT" : "TAXID-GI-OFFSET=EDIT, which the grain of this fold needs,") +
                                 " with numbers of 1 to 10 digits up to 4294967295 (" + std::to_string(ctr[kParseCtrFormat]) + " such tokens in this call)");
    {
        // (of the three refusals of the lines' order, the one with the first line)
        static const char* const what[3] = {"a key below the one before it: the tokens of a line must ascend by the key of the fold's grain",
                                            "line_read is not above the read of the non-empty line before it",
                                            "line_read is at or above the n_reads of the fold's last reset"};
        const uint32_t slot[3] = {kParseCtrKeyOrder, kParseCtrReadOrder, kParseCtrReadRange};
        int first = -1;
        for (int k = 0; k < 3; k++)
            if (ctr[slot[k]] && (first < 0 || ctr[slot[k] + 1] < ctr[slot[first] + 1])) first = k;
        if (first >= 0)
            throw std::runtime_error("arg: line " + std::to_string(ctr[slot[first] + 1]) + ": " + what[first] + " (" + std::to_string(ctr[slot[first]]) +
                                     " such places in this call)");
    }
    const uint64_t n_rec = ctr[kParseCounters + 1];
    if (!n_rec || n_rec > n_tok) throw std::runtime_error("internal: " + std::to_string(n_tok) + " tokens made " + std::to_string(n_rec) + " records");
    if (n + n_rec >= (1ull << 32)) throw std::runtime_error("limit: the fold would hold " + std::to_string(n + n_rec) + " records before equal keys are joined, 2^32 or more");
    // ---- the records, in the fold's incoming array; their TaxIDs for the union ----
    in_room(n_rec);
    P.d_tax.room(stream, n_rec, "the records' TaxIDs");
    HIP_CHECK(hipEventRecord(P.ev[4], stream));
    launch_parse_reduce(stream, grain, P.d_raw_key.p, P.d_raw_val.p, P.d_flag.p, P.d_place.p, (uint32_t)n_tok, (uint32_t)n_rec, d_in.p, P.d_tax.p);
    HIP_CHECK(hipEventRecord(P.ev[5], stream));
    taxa_in.resize(n_rec);
    HIP_CHECK(hipMemcpyAsync(taxa_in.data(), P.d_tax.p, n_rec * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    HIP_CHECK(hipGetLastError());
    std::sort(taxa_in.begin(), taxa_in.end());
    taxa_in.erase(std::unique(taxa_in.begin(), taxa_in.end()), taxa_in.end());
    float ms = 0, part = 0, fold_ms = 0;
    for (int k = 0; k < 6; k += 2) {
        HIP_CHECK(hipEventElapsedTime(&part, P.ev[k], P.ev[k + 1]));
        ms += part;
    }
    fold_in(n_rec, taxa_in, &fold_ms);
    HIP_CHECK(hipStreamSynchronize(stream));
    if (n_records) *n_records = n_rec;
    if (device_ms) *device_ms = ms + fold_ms;
    if (trace)
        fprintf(stderr, "[parse] %llu bytes in %llu lines -> %llu tokens -> %llu records in %u tiles of %u bytes: %.3f ms\n", (unsigned long long)N,
                (unsigned long long)n_lines, (unsigned long long)n_tok, (unsigned long long)n_rec, tiles, P.tile, ms);
    // MTSV_PARSE_TIMING=1: where a call spends its time (tools/collapse_ab.py reads this line)
    if (P.timing)
        fprintf(stderr, "[parse timing] bytes %llu lines %llu tokens %llu records %llu; upload %.3f ms, kernels %.3f ms, fold %.3f ms, call %.3f ms\n",
                (unsigned long long)N, (unsigned long long)n_lines, (unsigned long long)n_tok, (unsigned long long)n_rec, t1 - t0, ms, fold_ms, now_ms() - t0);
}

}  // namespace mtsv
