// parse.hpp -- result text that lies in HBM turned back into assignment records there (parse.hip, k_parse.hip).
#pragma once
#include "../../include/mtsv_amd.h"
#include "dev_mem.hpp"
#include "kernels.hpp"

namespace mtsv {

// What one call of mtsv_fold_add_text needs beside the fold's own arrays: the uploaded text, the lines' offsets and reads,
// the raw tokens and the scratch of the two scans.  A fold creates one on its first call and keeps it; its arrays grow by
// reallocation and are kept from call to call.  Everything runs on the fold's stream.
struct TextParser {
    int device;
    hipStream_t stream;         // the fold's
    uint32_t tile = kParseTile;  // MTSV_PARSE_TILE (tests): a power of two, 64 .. kParseTileMax
    bool trace = false, timing = false;
    DevEvents<6> ev;  // three pairs: count, tokens and heads, reduce
    DevBuf<uint8_t> d_hits;
    DevBuf<uint64_t> d_line_off;
    DevBuf<uint32_t> d_line_read;
    DevBuf<uint32_t> d_tile_cnt;
    DevBuf<uint32_t> d_tile_off;
    DevBuf<uint64_t> d_sums;  // the scans' tile sums
    DevBuf<uint64_t> d_ctr;   // kParseCounters, then the tokens, then the records
    DevBuf<uint8_t> d_raw_key;
    DevBuf<uint8_t> d_raw_val;
    DevBuf<uint32_t> d_flag;
    DevBuf<uint32_t> d_place;
    DevBuf<uint32_t> d_tax;  // the records' TaxIDs, for the host

    TextParser(int device, hipStream_t stream);
    ~TextParser();
    TextParser(const TextParser&) = delete;
    TextParser& operator=(const TextParser&) = delete;
};

}  // namespace mtsv
