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
#include "binner_run.hpp"

using namespace mtsv_cli;

int main(int argc, char** argv) {
    setup_mark("main");
    const Run run = resolve(parse_args(argc, argv));
    mtsv_ingest::keep_records() = run.partition;  // descriptions and qualities: only when records are written out again
    Producer producer(run);
    if (!producer.open()) {
        logmsg("ERROR", "Error running query: cannot open " + run.input);
        return 2;
    }
    if (run.parse_only) return parse_only(run, producer);
    Outputs outputs;
    if (const int c = outputs.open(run)) return c;
    logmsg("INFO", "Deserializing candidate filter ...");
    require_index_paths(run);
    return run.folded() ? run_folded(run, producer, outputs) : run_pipelined(run, producer, outputs);
}
