// parse.hpp -- result text that lies in HBM turned back into assignment records there (parse.hip, k_parse.hip).
#pragma once
#include "../../include/mtsv_amd.h"
#include "dev_index.hpp"
#include "kernels.hpp"

namespace mtsv {

// What one call of mtsv_fold_add_text needs beside the fold's own arrays: the uploaded text, the lines' offsets and reads,
// the raw tokens and the scratch of the two scans.  A fold creates one on its first call and keeps it; its arrays grow by
// reallocation and are kept from call to call.  Everything runs on the fold's stream.
struct TextParser {
    int device;
    hipStream_t stream;         // the fold's
    uint32_t tile = kParseTile;  // MTSV_PARSE_TILE (tests)
    bool trace = false, timing = false;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // three pairs: count, tokens and heads, reduce
    uint8_t* d_hits = nullptr;
    uint64_t* d_line_off = nullptr;
    uint32_t* d_line_read = nullptr;
    uint32_t* d_tile_cnt = nullptr;
    uint32_t* d_tile_off = nullptr;
    uint64_t* d_sums = nullptr;  // the scans' tile sums
    uint64_t* d_ctr = nullptr;   // kParseCounters, then the tokens, then the records
    uint8_t* d_raw_key = nullptr;
    uint8_t* d_raw_val = nullptr;
    uint32_t* d_flag = nullptr;
    uint32_t* d_place = nullptr;
    uint32_t* d_tax = nullptr;  // the records' TaxIDs, for the host
    uint64_t hits_cap = 0, off_cap = 0, read_cap = 0, cnt_cap = 0, toff_cap = 0, sums_cap = 0, ctr_cap = 0, key_cap = 0, val_cap = 0, flag_cap = 0,
             place_cap = 0, tax_cap = 0;

    TextParser(int device, hipStream_t stream);
    ~TextParser();
    TextParser(const TextParser&) = delete;
    TextParser& operator=(const TextParser&) = delete;

    // MTSV_PARSE_TILE as a tile size: a power of two, 64 .. kParseTileMax; kParseTile when it is not set
    static uint32_t tile_from_env();
};

}  // namespace mtsv
