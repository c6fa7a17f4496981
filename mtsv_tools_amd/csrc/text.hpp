// text.hpp -- the result lines of assignment records that lie in HBM, written there (text.hip, k_text.hip).
#pragma once
#include <vector>

#include "../../include/mtsv_amd.h"
#include "dev_mem.hpp"
#include "kernels.hpp"

namespace mtsv {

// Owns everything one call of mtsv_fold_format_text / mtsv_batch_format_text needs beside the records: the read IDs'
// upload, the scratch arrays, the three launches and the copy of the text to the host.  A fold or a workspace creates
// one on its first call and keeps it; its arrays grow by reallocation and are kept from call to call.
struct TextFormatter {
    int device;
    uint32_t tile = kTextTile;  // MTSV_TEXT_TILE (tests): a power of two, 2 .. kTextTileMax
    bool trace = false, timing = false;
    hipStream_t stream = nullptr;
    DevEvents<4> ev;
    DevBuf<uint8_t> d_ids;
    DevBuf<uint64_t> d_id_off;
    DevBuf<uint8_t> d_gather;  // records that lie in several stretches, next to each other
    DevBuf<uint32_t> d_rec_len;
    DevBuf<uint32_t> d_tile_cnt;
    DevBuf<uint64_t> d_tile_off;
    DevBuf<uint64_t> d_sums;  // the scan's sums, then the total, then the two counters of the measure pass
    DevBuf<uint8_t> d_out;

    explicit TextFormatter(int device);
    ~TextFormatter();
    TextFormatter(const TextFormatter&) = delete;
    TextFormatter& operator=(const TextFormatter&) = delete;

    struct Stretch {
        const uint8_t* rec;  // device memory
        uint64_t n;
    };
    // The lines of the records of `grain` in src (in order: together they are one list ordered by key; nothing of them is
    // in flight).  *text: page-locked, from the pool of result arrays, *len + 1 bytes with a NUL at *len.  Whatever fails
    // leaves nothing behind.
    void format(int grain, const std::vector<Stretch>& src, const char* ids, const uint64_t* id_off, uint64_t n_reads, char** text, uint64_t* len,
                float* device_ms);
};

}  // namespace mtsv
