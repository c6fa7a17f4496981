// binner_ingest.hpp -- the producer side of mtsv-binner (get_fastx_and_write_matching_bin_ids, binner.rs:149-217): the
// input file as blocks of reads, in input order, from recycled (page-locked) buffers.
#pragma once
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "binner_args.hpp"
#include "fastx_ingest.hpp"

namespace mtsv_cli {

using mtsv_ingest::ReadBlock;

// batches are recycled (writer -> producer) so that steady state touches no fresh pages
class BlockPool {
   public:
    std::unique_ptr<ReadBlock> get();
    void put(std::unique_ptr<ReadBlock> b);
    // a stock of blocks whose (page-locked) base buffers exist before the first query: creating one costs
    // milliseconds per block, which the first second of a run would otherwise spend in its parser threads
    void stock(size_t n, uint64_t base_bytes);

   private:
    std::mutex mu_;
    std::vector<std::unique_ptr<ReadBlock>> free_;
    size_t keep_ = 8;
};

// Parsed blocks in page-locked memory from here on (mtsv_host_alloc), which the GPU's copy engine reads in place -- unless
// MTSV_CLI_PAGEABLE is set or a batch would be larger than such a buffer should be.  True when installed.
bool install_pinned_blocks(uint64_t batch_reads);

// What the head of the input says (plain text only; a gzip head says nothing).
struct InputHead {
    double bytes_per_record = 0;  // over the first 256 KiB; 0: fewer than 8 records there
    uint32_t first_read_len = 0;  // the first read's bases, within the first 64 KiB; 0: not seen
};
InputHead sniff_head(const std::string& input, bool fastq);

class Producer {
   public:
    using Emit = std::function<bool(std::unique_ptr<ReadBlock>)>;
    explicit Producer(const Run& run) : run_(run) {}
    bool open();  // false: the input cannot be opened
    // Block-parallel ingest of plain and gzip files (fastx_ingest.hpp), the serial reader from the first irregular block on
    // (MTSV_SERIAL_INGEST=1: from the start).  The reads before run.read_offset are skipped; `emit` gets blocks of about
    // batch_reads reads in input order and stops the producer by returning false.  False: a read error, see error().
    bool produce(uint64_t batch_reads, const Emit& emit);
    const std::string& error() const { return rd_.err_msg; }
    // the length of the input's first read (plain text; 150 otherwise): the workspaces are sized and warmed with reads like it
    uint32_t warm_len() const { return head_.first_read_len >= 32 ? std::min<uint32_t>(head_.first_read_len, 1000) : 150; }

    BlockPool pool;
    std::function<void()> all_emitted;  // called once the last batch has been handed to emit, before the input is closed

   private:
    uint64_t ingest_block_bytes(uint64_t batch_reads) const;
    bool produce_serial(std::unique_ptr<ReadBlock> w, uint64_t skipped, uint64_t batch_reads, const Emit& emit);
    const Run& run_;
    mtsv_ingest::FastxReader rd_;  // the serial reader; its file is the one open() opened
    InputHead head_;
};

// --parse-only: the ingest self-check -- counts and FNV-1a checksums of everything the binner would see.  The exit code.
int parse_only(const Run& run, Producer& producer);

}  // namespace mtsv_cli
