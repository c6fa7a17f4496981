// binner_handles.hpp -- mtsv-binner's side of libmtsv_amd: owning handles, the run's exit code, workspace sizing.
#pragma once
#include <algorithm>
#include <memory>
#include <mutex>
#include <string>

#include "../../include/mtsv_amd.h"
#include "cli_common.hpp"

namespace mtsv_cli {

inline void logmsg(const char* level, const std::string& msg) { logmsg("mtsv_binner", level, msg); }

// A handle frees itself when it goes out of scope: an error path is "log, set the code, return", and mtsv_last_error()
// (thread-local) has been read by then.
struct IndexFree {
    void operator()(mtsv_index* q) const { mtsv_index_free(q); }
};
struct BatchFree {
    void operator()(mtsv_batch* q) const { mtsv_batch_free(q); }
};
struct FoldFree {
    void operator()(mtsv_fold* q) const { mtsv_fold_free(q); }
};
struct DupmapFree {
    void operator()(mtsv_dupmap* q) const { mtsv_dupmap_free(q); }
};
struct CoverageFree {
    void operator()(mtsv_coverage* q) const { mtsv_coverage_free(q); }
};
struct PileupFree {
    void operator()(mtsv_pileup* q) const { mtsv_pileup_free(q); }
};
struct ArrayFree {
    void operator()(void* q) const { mtsv_free(q); }
};
using IndexPtr = std::unique_ptr<mtsv_index, IndexFree>;
using BatchPtr = std::unique_ptr<mtsv_batch, BatchFree>;
using FoldPtr = std::unique_ptr<mtsv_fold, FoldFree>;
using DupmapPtr = std::unique_ptr<mtsv_dupmap, DupmapFree>;
using CoveragePtr = std::unique_ptr<mtsv_coverage, CoverageFree>;
using PileupPtr = std::unique_ptr<mtsv_pileup, PileupFree>;
template <class T>
using ArrayPtr = std::unique_ptr<T, ArrayFree>;  // what the library hands out for mtsv_free

// for the library's `T** out` parameters: receives into a raw pointer and hands it to the owner at the end of the full
// expression the call stands in -- so the owner is read in a LATER statement, never further along in the same one
template <class P>
class Receiver {
   public:
    explicit Receiver(P& owner) : owner_(owner) {}
    ~Receiver() { owner_.reset(raw_); }
    operator typename P::pointer*() { return &raw_; }

   private:
    P& owner_;
    typename P::pointer raw_ = nullptr;
};
template <class P>
Receiver<P> out(P& owner) {
    return Receiver<P>(owner);
}

// The exit code of a run: the first failure's, from whichever thread.  lib_error() is called on the thread whose library
// call failed, before anything else is called there (the message is that thread's).
class ExitCode {
   public:
    void set(int c) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!code_) code_ = c;
    }
    int get() {
        std::lock_guard<std::mutex> lk(mu_);
        return code_;
    }
    bool failed() { return get() != 0; }
    bool lib_error() { return lib_error(mtsv_last_error()); }
    bool lib_error(const std::string& msg) {  // (a message taken on another thread)
        logmsg("ERROR", "Error running query: " + msg);
        set(2);
        return false;
    }

   private:
    std::mutex mu_;
    int code_ = 0;
};

// A parser block holds up to one and a half batches (binner_ingest.cpp: "the block is the batch").
inline uint64_t block_reads_max(uint64_t batch_reads) { return batch_reads + batch_reads / 2; }
// The reads of one library call of the pipelined run: a group and the block that overshoots it.
inline uint64_t call_reads_max(uint64_t group_reads, uint64_t batch_reads) { return group_reads + block_reads_max(batch_reads); }
// Bases of a workspace that holds `reads` reads like the input's first (read_len bases) as one resident batch.
inline uint64_t workspace_bases(uint64_t reads, uint32_t read_len, uint64_t at_least) {
    return std::min<uint64_t>(3ull << 30, std::max<uint64_t>(reads * std::max<uint64_t>(512, 2 * (uint64_t)read_len), at_least));
}

}  // namespace mtsv_cli
