// binner_run.hpp -- the two runs of mtsv-binner.  Both take a validated command line, the producer with its input open and
// the output files open, and return the exit code -- or leave the process themselves once the results are on their way to
// the disk (MTSV_CLI_CLEAN_EXIT=1: they return, and free what they hold).
#pragma once
#include "binner_args.hpp"
#include "binner_handles.hpp"
#include "binner_ingest.hpp"
#include "binner_outputs.hpp"

namespace mtsv_cli {

int run_folded(const Run& run, Producer& producer, Outputs& outputs);     // --fold-on-gpu (binner_fold.cpp)
int run_pipelined(const Run& run, Producer& producer, Outputs& outputs);  // every other mode (binner_pipeline.cpp)

}  // namespace mtsv_cli
