"""mtsv_tools_amd -- MI355X-native mtsv-binner hot path.

The product is the C-ABI shared library ``libmtsv_amd.so`` (C++ host + hand-written HIP kernels
for gfx950, built in-tree from ``mtsv_tools_amd/csrc``; interface in ``include/mtsv_amd.h``).
This Python package is only a thin ctypes harness over that ABI for tests and ``bench.py``; it
holds no algorithm and has no CPU fallback: every call that needs the GPU raises ``MtsvError``
when the library or a device is missing.
"""
from ._lib import (  # noqa: F401
    ASSIGN_DTYPE,
    ASSIGN_GI_DTYPE,
    ASSIGN_OFF,
    ASSIGN_ONLY,
    ASSIGN_WITH_HITS,
    CLADE_STATS_DTYPE,
    Coverage,
    DEVPART_BIN_END,
    DEVPART_BIN_LUT,
    DEVPART_BINS,
    DEVPART_BLOCKS,
    DEVPART_HEADER,
    DEVPART_SA_SAMPLE,
    DEVPART_TEXT,
    DEVPART_TEXT_SECTORS,
    DeviceHeader,
    GRAIN_LONG,
    GRAIN_TAXID,
    GRAIN_TAXID_GI,
    HIT_DTYPE,
    KEEP_MATCHED,
    KEEP_UNMATCHED,
    MATCH_OFF,
    MATCH_ONLY,
    MATCH_WITH_HITS,
    RANK_UNKNOWN,
    REF_COVERAGE_DTYPE,
    SLACK_ALL,
    TAXON_STATS_DTYPE,
    Taxonomy,
    HostBuffer,
    host_register,
    host_unregister,
    Batch,
    DupMap,
    Fold,
    MGIndex,
    MtsvError,
    PAIR_BOTH,
    PAIR_EITHER,
    PAIR_PROPER,
    PairStats,
    Params,
    bin_batch_chunks,
    bin_batch_multi,
    bin_batch_slice_reads,
    default_params,
    device_count,
    format_assignments,
    format_assignments_gi,
    format_clade_report,
    format_coverage_report,
    format_results,
    format_taxa_report,
    merge_taxa_reports,
    lib,
    lib_path,
    pack_bases,
    set_build_device,
    synth_reads,
    version,
)

DEV_DEFAULT = 0
DEV_SAMPLED_SA_ONLY = 1
DEV_NO_KMER_TABLE = 2
DEV_PACK_ON_DEVICE = 4
