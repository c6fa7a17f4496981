"""ctypes binding of libmtsv_amd.so (include/mtsv_amd.h).  No algorithm lives here."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # MTSV_AMD_LIB: a variant build of the same library (tools/build_variant.sh, kernel experiments)
    return os.environ.get("MTSV_AMD_LIB") or os.path.join(_HERE, "libmtsv_amd.so")


class MtsvError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mtsv error {code}: {msg}")
        self.code = code


E_ARG, E_IO, E_FORMAT, E_DEVICE, E_LIMIT, E_NOMEM = -1, -2, -3, -4, -5, -6
MATCH_OFF, MATCH_WITH_HITS, MATCH_ONLY = 0, 1, 2  # MTSV_MATCH_*
ASSIGN_OFF, ASSIGN_WITH_HITS, ASSIGN_ONLY = 0, 1, 2  # MTSV_ASSIGN_*
GRAIN_TAXID, GRAIN_TAXID_GI, GRAIN_LONG = 0, 1, 2  # MTSV_GRAIN_*
KEEP_UNMATCHED, KEEP_MATCHED = 0, 1  # MTSV_KEEP_*
# MTSV_DEVPART_*
DEVPART_HEADER, DEVPART_BLOCKS, DEVPART_TEXT, DEVPART_SA_SAMPLE, DEVPART_BINS, DEVPART_BIN_END, DEVPART_BIN_LUT, DEVPART_TEXT_SECTORS = range(8)


class Params(C.Structure):  # mtsv_params
    _fields_ = [("edit_rate", C.c_double), ("seed_size", C.c_uint32), ("seed_interval", C.c_uint32),
                ("min_seed", C.c_double), ("max_hits", C.c_uint64), ("tune_max_hits", C.c_uint64),
                ("max_assignments", C.c_int64), ("max_candidates", C.c_int64)]


class IndexInfo(C.Structure):  # mtsv_index_info_t
    _fields_ = [("n", C.c_uint64), ("n_bins", C.c_uint64), ("occ_k", C.c_uint32),
                ("sa_s", C.c_uint64), ("file_bytes", C.c_uint64), ("device_bytes", C.c_uint64),
                ("kmer_k", C.c_uint32), ("sa_full", C.c_uint32)]


class DeviceHeader(C.Structure):  # mtsv_device_header
    _fields_ = [("n", C.c_uint32), ("n_blocks", C.c_uint32), ("C", C.c_uint32 * 5), ("sentinel_row", C.c_uint32),
                ("sa_s", C.c_uint32), ("sa_pow2_shift", C.c_uint32), ("n_bins", C.c_uint32), ("bin_lut_shift", C.c_uint32),
                ("kmer_k", C.c_uint32), ("sa_full", C.c_uint32), ("packed_on_device", C.c_uint32), ("_pad", C.c_uint32),
                ("device_bytes", C.c_uint64), ("pack_ms", C.c_float), ("copy_ms", C.c_float), ("accel_build_ms", C.c_float),
                ("_pad2", C.c_float)]


N_STAGES = 8
STAGE_NAMES = ("search", "thin_scan", "expand", "locate", "coalesce", "verify", "gather", "total")


class BatchStats(C.Structure):  # mtsv_batch_stats
    _fields_ = [("stage_ms", C.c_float * N_STAGES), ("n_reads", C.c_uint64),
                ("n_seed_slots", C.c_uint64), ("n_seed_hits", C.c_uint64), ("lf_steps", C.c_uint64),
                ("n_candidates", C.c_uint64), ("n_verified", C.c_uint64),
                ("window_bytes", C.c_uint64), ("n_hits", C.c_uint64), ("n_passes", C.c_uint64),
                ("n_rounds", C.c_uint64), ("n_lanes", C.c_uint64), ("sw_cell_pairs", C.c_uint64), ("sw_prefilter_ms", C.c_float),
                ("sw_sweep_ms", C.c_float), ("n_sw_passed", C.c_uint64), ("sw_diag_ms", C.c_float), ("sw_bound_ms", C.c_float),
                ("edit_ms", C.c_float), ("myers_columns", C.c_uint64), ("n_sw_bound_refuted", C.c_uint64),
                ("verify_turns", C.c_uint64), ("verify_lanes_max", C.c_uint64), ("myers_grid_max", C.c_uint64),
                ("n_seed_tile_passes", C.c_uint64)]

    def as_dict(self):
        d = {n: (float(getattr(self, n)) if t is C.c_float else int(getattr(self, n))) for n, t in self._fields_[1:]}
        d["stage_ms"] = {STAGE_NAMES[i]: float(self.stage_ms[i]) for i in range(N_STAGES)}
        return d


# mtsv_hit: 8 + 4 + 4 + 4 + 1 + 3 pad + 8 = 32 bytes
HIT_DTYPE = np.dtype({"names": ["read", "tax_id", "gi", "edit", "strand", "offset"],
                      "formats": ["<u8", "<u4", "<u4", "<u4", "u1", "<u8"],
                      "offsets": [0, 8, 12, 16, 20, 24], "itemsize": 32})

# mtsv_taxon_stats: 4 + 4 pad + 4 * 8 = 40 bytes
TAXON_STATS_DTYPE = np.dtype({"names": ["tax_id", "only_hit", "only_best", "tied_best", "not_best"],
                              "formats": ["<u4", "<u8", "<u8", "<u8", "<u8"],
                              "offsets": [0, 8, 16, 24, 32], "itemsize": 40})

# mtsv_assignment: 8 + 4 + 4 = 16 bytes
ASSIGN_DTYPE = np.dtype({"names": ["read", "tax_id", "edit"], "formats": ["<u8", "<u4", "<u4"], "offsets": [0, 8, 12], "itemsize": 16})

# mtsv_assignment_gi: 8 + 4 * 4 = 24 bytes
ASSIGN_GI_DTYPE = np.dtype({"names": ["read", "tax_id", "gi", "offset", "edit"], "formats": ["<u8", "<u4", "<u4", "<u4", "<u4"],
                            "offsets": [0, 8, 12, 16, 20], "itemsize": 24})

# mtsv_clade_stats: 4 * 4 + 2 * 8 = 32 bytes
CLADE_STATS_DTYPE = np.dtype({"names": ["tax_id", "parent_tax_id", "rank", "depth", "direct", "clade"],
                              "formats": ["<u4", "<u4", "<u4", "<u4", "<u8", "<u8"], "offsets": [0, 4, 8, 12, 16, 24], "itemsize": 32})
RANK_UNKNOWN = 0xffffffff  # MTSV_RANK_UNKNOWN
SLACK_ALL = 0xffffffff  # edit_slack of mtsv_fold_lca: every TaxID of a read enters
PAIR_BOTH, PAIR_EITHER, PAIR_PROPER = 0, 1, 2  # MTSV_PAIR_*

# mtsv_abundance_row: 4 + 4 pad + 4 * 8 = 40 bytes
ABUNDANCE_ROW_DTYPE = np.dtype({"names": ["tax_id", "mass", "reads_any", "reads_unique", "assigned"], "formats": ["<u4", "<u8", "<u8", "<u8", "<u8"],
                                "offsets": [0, 8, 16, 24, 32], "itemsize": 40})

# mtsv_ref_coverage: 4 + 4 + 5 * 8 = 48 bytes
REF_COVERAGE_DTYPE = np.dtype({"names": ["tax_id", "gi", "length", "reads", "alignments", "aligned_bases", "covered_bases"],
                               "formats": ["<u4", "<u4", "<u8", "<u8", "<u8", "<u8", "<u8"], "offsets": [0, 4, 8, 16, 24, 32, 40], "itemsize": 48})

# mtsv_placement: 8 + 3 * 4 + 1 + 3 pad + 3 * 4 + 4 pad + 8 = 48 bytes
PLACEMENT_DTYPE = np.dtype({"names": ["read", "tax_id", "gi", "edit", "strand", "ref_start", "ref_end", "n_ops", "ops_off"],
                            "formats": ["<u8", "<u4", "<u4", "<u4", "u1", "<u4", "<u4", "<u4", "<u8"],
                            "offsets": [0, 8, 12, 16, 20, 24, 28, 32, 40], "itemsize": 48})
CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X = 1, 2, 7, 8  # BAM's op codes: an op is len << 4 | code

# mtsv_pile_site: 3 * 4 + 1 + 3 pad + 8 * 4 = 48 bytes; n: match, A, C, G, T, N, del, ins
PILE_SITE_DTYPE = np.dtype({"names": ["tax_id", "gi", "pos", "ref", "n"], "formats": ["<u4", "<u4", "<u4", "u1", ("<u4", (8,))],
                            "offsets": [0, 4, 8, 12, 16], "itemsize": 48})
PILE_REF_NONE = 0xff  # the ref code of a reference's last slot, which takes insertions only

# mtsv_cons_ref: 10 * 4 + 8 = 48 bytes
CONS_REF_DTYPE = np.dtype({"names": ["tax_id", "gi", "length", "covered", "n_ref", "n_sub", "n_del", "n_low", "n_ambig", "ins_sites", "sum_depth"],
                           "formats": ["<u4"] * 10 + ["<u8"], "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40], "itemsize": 48})
CONS_FILL_N, CONS_FILL_REF = 0, 1


class PileupInfo(C.Structure):  # mtsv_pileup_info_t
    _fields_ = [("n_refs", C.c_uint64), ("n_slots", C.c_uint64), ("n_segments", C.c_uint64), ("device_bytes", C.c_uint64),
                ("hits_piled", C.c_uint64), ("hits_skipped", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class TaxonomyInfo(C.Structure):  # mtsv_taxonomy_info_t
    _fields_ = [("n_nodes", C.c_uint64), ("n_implied_roots", C.c_uint64), ("n_ranks", C.c_uint32), ("max_depth", C.c_uint32)]


class AbundanceInfo(C.Structure):  # mtsv_abundance_info: 5 * 8 + 2 * 4 = 48 bytes
    _fields_ = [("reads", C.c_uint64), ("entries", C.c_uint64), ("taxa", C.c_uint64), ("total_mass", C.c_uint64), ("l1_change", C.c_uint64),
                ("iterations", C.c_uint32), ("converged", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PairStats(C.Structure):  # mtsv_pair_stats
    _fields_ = [("pairs", C.c_uint64), ("both_mates_hit", C.c_uint64), ("one_mate_hit", C.c_uint64), ("joined", C.c_uint64),
                ("records", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


EXPORTS = [
    "mtsv_last_error", "mtsv_version", "mtsv_params_default", "mtsv_device_count",
    "mtsv_index_load", "mtsv_index_build", "mtsv_index_build_fasta", "mtsv_index_write",
    "mtsv_index_info", "mtsv_index_free", "mtsv_set_build_device", "mtsv_index_to_device", "mtsv_bin_batch",
    "mtsv_hits_free", "mtsv_batch_create", "mtsv_batch_upload", "mtsv_batch_run", "mtsv_batch_run_host", "mtsv_batch_run_host_parts",
    "mtsv_batch_stats_get", "mtsv_batch_set_verify_mode", "mtsv_batch_download", "mtsv_batch_free", "mtsv_format_results",
    "mtsv_free", "mtsv_synth_index", "mtsv_synth_reads", "mtsv_bin_batch_workspace_reads",
    "mtsv_bin_batch_multi", "mtsv_bin_batch_chunks", "mtsv_set_default_verify_mode",
    "mtsv_host_alloc", "mtsv_host_free", "mtsv_host_register", "mtsv_host_unregister",
    "mtsv_batch_create_lanes", "mtsv_batch_reserve_host", "mtsv_pack_bases", "mtsv_host_pack_threads",
    "mtsv_batch_set_taxa_report", "mtsv_batch_taxa_report", "mtsv_merge_taxa_reports", "mtsv_format_taxa_report",
    "mtsv_batch_set_match_flags", "mtsv_batch_match_flags",
    "mtsv_batch_take_reads", "mtsv_batch_read_map", "mtsv_batch_download_reads",
    "mtsv_batch_copy_reads", "mtsv_batch_merge_runs",
    "mtsv_batch_set_assignments", "mtsv_batch_download_assignments", "mtsv_format_assignments",
    "mtsv_batch_set_assignment_grain", "mtsv_batch_download_assignments_gi", "mtsv_format_assignments_gi",
    "mtsv_fold_create", "mtsv_fold_free", "mtsv_fold_reset", "mtsv_fold_add_run", "mtsv_fold_add_records", "mtsv_fold_count",
    "mtsv_fold_download", "mtsv_fold_download_gi", "mtsv_fold_taxa_report", "mtsv_fold_match_flags",
    "mtsv_fold_format_text", "mtsv_batch_format_text",
    "mtsv_index_download_device",
    "mtsv_fold_add_text",
    "mtsv_taxonomy_load", "mtsv_taxonomy_free", "mtsv_taxonomy_info", "mtsv_taxonomy_parent", "mtsv_taxonomy_rank_name",
    "mtsv_fold_lca", "mtsv_format_clade_report",
    "mtsv_dupmap_create", "mtsv_dupmap_free", "mtsv_batch_take_unique", "mtsv_dupmap_download", "mtsv_fold_expand",
    "mtsv_fold_pair",
    "mtsv_fold_abundance", "mtsv_abundance_weights", "mtsv_format_abundance",
    "mtsv_coverage_create", "mtsv_coverage_free", "mtsv_coverage_add_index", "mtsv_coverage_add_refs", "mtsv_coverage_reset",
    "mtsv_coverage_add_fold", "mtsv_coverage_rows", "mtsv_format_coverage_report",
    "mtsv_batch_place_hits", "mtsv_format_placements",
    "mtsv_pileup_create", "mtsv_pileup_free", "mtsv_pileup_reset", "mtsv_pileup_add_run", "mtsv_pileup_info", "mtsv_pileup_download",
    "mtsv_pileup_sites", "mtsv_format_variants",
    "mtsv_pileup_consensus", "mtsv_format_consensus_stats", "mtsv_pileup_add_counts",
]

_lib = None


def lib():
    """Load libmtsv_amd.so; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise MtsvError(E_DEVICE, f"{p} is missing: run `make -C mtsv_tools_amd/csrc` "
                                      "(or __graft_entry__.build()); there is no fallback path")
        L = C.CDLL(p)
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.mtsv_last_error.restype = C.c_char_p
        L.mtsv_version.restype = C.c_char_p
        L.mtsv_params_default.argtypes = [C.POINTER(Params)]
        L.mtsv_index_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.mtsv_index_build.argtypes = [u64, vp, vp, vp, vp, u32, u64, i32, C.POINTER(vp)]
        L.mtsv_index_build_fasta.argtypes = [C.c_char_p, u32, u64, i32, C.POINTER(vp)]
        L.mtsv_index_write.argtypes = [vp, C.c_char_p]
        L.mtsv_index_info.argtypes = [vp, C.POINTER(IndexInfo)]
        L.mtsv_index_free.argtypes = [vp]
        L.mtsv_index_free.restype = None
        L.mtsv_index_to_device.argtypes = [vp, i32, u32]
        L.mtsv_index_download_device.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_bin_batch.argtypes = [vp, i32, vp, vp, u64, C.POINTER(Params), C.POINTER(vp),
                                     C.POINTER(u64)]
        L.mtsv_hits_free.argtypes = [vp]
        L.mtsv_hits_free.restype = None
        L.mtsv_bin_batch_multi.argtypes = [vp, vp, i32, vp, vp, u64, C.POINTER(Params), C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_bin_batch_chunks.argtypes = [vp, vp, i32, vp, vp, u64, C.POINTER(Params), C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_bin_batch_workspace_reads.argtypes = [u64]
        L.mtsv_bin_batch_workspace_reads.restype = u64
        L.mtsv_batch_create.argtypes = [vp, i32, u64, u64, u64, C.POINTER(vp)]
        L.mtsv_batch_create_lanes.argtypes = [vp, i32, u64, u64, u64, i32, C.POINTER(vp)]
        L.mtsv_batch_reserve_host.argtypes = [vp, u64, u64, u32]
        L.mtsv_pack_bases.argtypes = [vp, vp, u64, u64, C.c_uint8]
        L.mtsv_pack_bases.restype = C.c_uint8
        L.mtsv_batch_upload.argtypes = [vp, vp, vp, u64]
        L.mtsv_batch_run.argtypes = [vp, C.POINTER(Params)]
        L.mtsv_batch_run_host.argtypes = [vp, vp, vp, u64, C.POINTER(Params)]
        L.mtsv_batch_run_host_parts.argtypes = [vp, i32, vp, vp, vp, C.POINTER(Params)]
        L.mtsv_batch_set_verify_mode.argtypes = [vp, i32]
        L.mtsv_batch_stats_get.argtypes = [vp, C.POINTER(BatchStats)]
        L.mtsv_batch_download.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_batch_free.argtypes = [vp]
        L.mtsv_batch_free.restype = None
        L.mtsv_format_results.argtypes = [vp, u64, C.c_char_p, vp, u64, i32, C.POINTER(vp),
                                          C.POINTER(u64)]
        L.mtsv_free.argtypes = [vp]
        L.mtsv_free.restype = None
        L.mtsv_synth_index.argtypes = [u64, u32, u32, u64, u32, u64, i32, C.POINTER(vp)]
        L.mtsv_synth_reads.argtypes = [vp, u64, u64, u32, vp, vp]
        L.mtsv_host_alloc.argtypes = [C.c_size_t]
        L.mtsv_host_alloc.restype = vp
        L.mtsv_host_free.argtypes = [vp]
        L.mtsv_host_free.restype = None
        L.mtsv_host_register.argtypes = [vp, C.c_size_t]
        L.mtsv_host_unregister.argtypes = [vp]
        L.mtsv_batch_set_taxa_report.argtypes = [vp, i32]
        L.mtsv_batch_taxa_report.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float), i32]
        L.mtsv_merge_taxa_reports.argtypes = [vp, u64, vp, u64, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_format_taxa_report.argtypes = [vp, u64, u64, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_batch_set_match_flags.argtypes = [vp, i32]
        L.mtsv_batch_match_flags.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
        L.mtsv_batch_take_reads.argtypes = [vp, vp, i32, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_batch_copy_reads.argtypes = [vp, vp, C.POINTER(C.c_float)]
        L.mtsv_batch_merge_runs.argtypes = [vp, vp, i32, C.POINTER(C.c_float)]
        L.mtsv_batch_read_map.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_batch_download_reads.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_batch_set_assignments.argtypes = [vp, i32]
        L.mtsv_batch_download_assignments.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_format_assignments.argtypes = [vp, u64, C.c_char_p, vp, u64, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_batch_set_assignment_grain.argtypes = [vp, i32]
        L.mtsv_batch_download_assignments_gi.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_format_assignments_gi.argtypes = [vp, u64, C.c_char_p, vp, u64, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_fold_create.argtypes = [i32, i32, C.POINTER(vp)]
        L.mtsv_fold_free.argtypes = [vp]
        L.mtsv_fold_free.restype = None
        L.mtsv_fold_reset.argtypes = [vp, u64]
        L.mtsv_fold_add_run.argtypes = [vp, vp, C.POINTER(C.c_float)]
        L.mtsv_fold_add_records.argtypes = [vp, vp, u64, C.POINTER(C.c_float)]
        L.mtsv_fold_count.argtypes = [vp, C.POINTER(u64)]
        L.mtsv_fold_download.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_fold_download_gi.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_fold_taxa_report.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_fold_match_flags.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
        L.mtsv_fold_format_text.argtypes = [vp, C.c_char_p, vp, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_batch_format_text.argtypes = [vp, C.c_char_p, vp, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_fold_add_text.argtypes = [vp, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_taxonomy_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.mtsv_taxonomy_free.argtypes = [vp]
        L.mtsv_taxonomy_free.restype = None
        L.mtsv_taxonomy_info.argtypes = [vp, C.POINTER(TaxonomyInfo)]
        L.mtsv_taxonomy_parent.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32)]
        L.mtsv_taxonomy_rank_name.argtypes = [vp, u32]
        L.mtsv_taxonomy_rank_name.restype = C.c_char_p
        L.mtsv_fold_lca.argtypes = [vp, vp, u32, vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_format_clade_report.argtypes = [vp, u64, u64, vp, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_fold_abundance.argtypes = [vp, vp, u32, u32, u32, u64, vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(AbundanceInfo), C.POINTER(C.c_float)]
        L.mtsv_abundance_weights.argtypes = [C.c_double, u32, vp]
        L.mtsv_format_abundance.argtypes = [vp, u64, C.POINTER(AbundanceInfo), C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_dupmap_create.argtypes = [i32, C.POINTER(vp)]
        L.mtsv_dupmap_free.argtypes = [vp]
        L.mtsv_dupmap_free.restype = None
        L.mtsv_batch_take_unique.argtypes = [vp, vp, vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_dupmap_download.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
        L.mtsv_fold_expand.argtypes = [vp, vp, vp, C.POINTER(C.c_float)]
        L.mtsv_fold_pair.argtypes = [vp, i32, u32, u32, vp, C.POINTER(PairStats), C.POINTER(C.c_float)]
        L.mtsv_coverage_create.argtypes = [i32, C.POINTER(vp)]
        L.mtsv_coverage_free.argtypes = [vp]
        L.mtsv_coverage_free.restype = None
        L.mtsv_coverage_add_index.argtypes = [vp, vp]
        L.mtsv_coverage_add_refs.argtypes = [vp, vp, vp, vp, u64]
        L.mtsv_coverage_reset.argtypes = [vp]
        L.mtsv_coverage_add_fold.argtypes = [vp, vp, vp, u64, u32, C.POINTER(C.c_float)]
        L.mtsv_coverage_rows.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_format_coverage_report.argtypes = [vp, u64, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_batch_place_hits.argtypes = [vp, vp, u64, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_format_placements.argtypes = [vp, u64, vp, C.c_char_p, vp, u64, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_pileup_create.argtypes = [i32, vp, u64, C.POINTER(vp)]
        L.mtsv_pileup_free.argtypes = [vp]
        L.mtsv_pileup_free.restype = None
        L.mtsv_pileup_reset.argtypes = [vp]
        L.mtsv_pileup_add_run.argtypes = [vp, vp, vp, u64, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_pileup_info.argtypes = [vp, C.POINTER(PileupInfo)]
        L.mtsv_pileup_download.argtypes = [vp, u32, u32, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_pileup_sites.argtypes = [vp, u32, u32, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_pileup_consensus.argtypes = [vp, u32, u32, u32, u32, u32, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), C.POINTER(C.c_float)]
        L.mtsv_format_consensus_stats.argtypes = [vp, u64, C.POINTER(vp), C.POINTER(u64)]
        L.mtsv_pileup_add_counts.argtypes = [vp, u32, u32, u32, u64, vp, u64]
        L.mtsv_format_variants.argtypes = [vp, u64, C.POINTER(vp), C.POINTER(u64)]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise MtsvError(rc, lib().mtsv_last_error().decode(errors="replace"))


def version():
    return lib().mtsv_version().decode()


def device_count():
    return lib().mtsv_device_count()


def bin_batch_multi(index, devices, bases, read_off, params=None):
    """mtsv_bin_batch_multi: one index replicated on `devices`, reads in contiguous blocks (Mode A)"""
    params = params or default_params()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
    dev = (C.c_int * len(devices))(*devices)
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_bin_batch_multi(index.h, dev, len(devices), bases.ctypes.data, read_off.ctypes.data,
                                      len(read_off) - 1, C.byref(params), C.byref(out), C.byref(n)))
    return _hits_from(out, n.value)


def bin_batch_chunks(indexes, devices, bases, read_off, params=None):
    """mtsv_bin_batch_chunks: chunk k of the database on devices[k], hit lists merged per read (Mode B)"""
    params = params or default_params()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
    dev = (C.c_int * len(devices))(*devices)
    hs = (C.c_void_p * len(indexes))(*[ix.h for ix in indexes])
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_bin_batch_chunks(hs, dev, len(indexes), bases.ctypes.data, read_off.ctypes.data,
                                       len(read_off) - 1, C.byref(params), C.byref(out), C.byref(n)))
    return _hits_from(out, n.value)


class HostBuffer:
    """mtsv_host_alloc: page-locked host memory as a uint8 numpy array (`.array`); free with close()"""

    def __init__(self, nbytes):
        self.ptr = lib().mtsv_host_alloc(nbytes)
        if not self.ptr:
            raise MtsvError(E_DEVICE, lib().mtsv_last_error().decode(errors="replace"))
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(1, nbytes)).from_address(self.ptr))[:nbytes]

    def close(self):
        if self.ptr:
            self.array = None
            lib().mtsv_host_free(self.ptr)
            self.ptr = None


def pack_bases(bases, first_offset=0, prev_code=0):
    """mtsv_pack_bases: the transfer format of run_host (4-bit codes, two per byte) of a uint8 array of bases that starts
    at segment offset first_offset; returns (packed bytes, code of the last base)"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    n = len(bases)
    out = np.zeros(((first_offset + n + 1) >> 1) - (first_offset >> 1) + 1, dtype=np.uint8)
    last = lib().mtsv_pack_bases(out.ctypes.data, bases.ctypes.data, first_offset, n, prev_code)
    return out[:-1], last


def host_register(arr):
    """page-lock the memory of a contiguous numpy array in place (mtsv_host_register); undo with host_unregister"""
    _check(lib().mtsv_host_register(arr.ctypes.data, arr.nbytes))


def host_unregister(arr):
    _check(lib().mtsv_host_unregister(arr.ctypes.data))


def bin_batch_slice_reads(n_reads):
    """reads per device workspace mtsv_bin_batch would create for a host batch of n_reads reads"""
    return int(lib().mtsv_bin_batch_workspace_reads(n_reads))


def set_build_device(device):
    """-1 = host suffix sort, >= 0 = GPU prefix doubling on that device (same index bytes)"""
    lib().mtsv_set_build_device.argtypes = [C.c_int]
    _check(lib().mtsv_set_build_device(device))


def default_params(**over):
    p = Params()
    lib().mtsv_params_default(C.byref(p))
    names = {f[0] for f in Params._fields_}
    for k, v in over.items():
        if k not in names:
            raise AttributeError(f"no such parameter: {k}")
        setattr(p, k, -1 if v is None else v)
    return p


def _hits_from(ptr, n):
    try:
        if n == 0:
            return np.zeros(0, dtype=HIT_DTYPE)
        raw = (C.c_ubyte * (n * HIT_DTYPE.itemsize)).from_address(ptr.value)
        return np.frombuffer(raw, dtype=HIT_DTYPE).copy()   # one copy, then the C array is freed
    finally:
        lib().mtsv_hits_free(ptr)


class MGIndex:
    """Owning handle of an mtsv_index (host MG-index + per-device HBM layout)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def load(cls, path):
        h = C.c_void_p()
        _check(lib().mtsv_index_load(os.fsencode(path), C.byref(h)))
        return cls(h)

    @classmethod
    def build(cls, entries, occ_k=64, sa_s=32, threads=4):
        entries = list(entries)
        n = len(entries)
        tax = np.array([e[0] for e in entries], dtype=np.uint32)
        gi = np.array([e[1] for e in entries], dtype=np.uint32)
        bufs = [C.create_string_buffer(bytes(e[2]), max(len(e[2]), 1)) for e in entries]
        ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(b) for b in bufs])
        lens = np.array([len(e[2]) for e in entries], dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().mtsv_index_build(n, tax.ctypes.data, gi.ctypes.data, ptrs, lens.ctypes.data,
                                      occ_k, sa_s, threads, C.byref(h)))
        return cls(h)

    @classmethod
    def build_fasta(cls, path, occ_k=64, sa_s=32, threads=4):
        h = C.c_void_p()
        _check(lib().mtsv_index_build_fasta(os.fsencode(path), occ_k, sa_s, threads, C.byref(h)))
        return cls(h)

    @classmethod
    def synth(cls, seed, n_taxa, gis_per_taxon, seq_len, occ_k=64, sa_s=32, threads=8):
        h = C.c_void_p()
        _check(lib().mtsv_synth_index(seed, n_taxa, gis_per_taxon, seq_len, occ_k, sa_s, threads,
                                      C.byref(h)))
        return cls(h)

    def write(self, path):
        _check(lib().mtsv_index_write(self.h, os.fsencode(path)))

    def info(self):
        i = IndexInfo()
        _check(lib().mtsv_index_info(self.h, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in i._fields_}

    def to_device(self, device=0, flags=0):
        _check(lib().mtsv_index_to_device(self.h, device, flags))

    def download_device(self, device=0, part=DEVPART_HEADER):
        """mtsv_index_download_device (for tests): the resident array `part` as bytes; DEVPART_HEADER as a dict of the
        scalars of mtsv_device_header (C as a list)"""
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().mtsv_index_download_device(self.h, device, part, C.byref(out), C.byref(n)))
        try:
            raw = C.string_at(out.value, n.value)
        finally:
            lib().mtsv_free(out)
        if part != DEVPART_HEADER:
            return raw
        h = DeviceHeader.from_buffer_copy(raw)
        d = {}
        for name, t in h._fields_:
            if name.startswith("_"):
                continue
            v = getattr(h, name)
            d[name] = list(v) if name == "C" else float(v) if t is C.c_float else int(v)
        return d

    def bin_batch(self, bases, read_off, params=None, device=0):
        """mtsv_bin_batch: hits ordered by (read, strand, rank)."""
        params = params or default_params()
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().mtsv_bin_batch(self.h, device, bases.ctypes.data, read_off.ctypes.data,
                                    len(read_off) - 1, C.byref(params), C.byref(out), C.byref(n)))
        return _hits_from(out, n.value)

    def close(self):
        if self.h is not None and _lib is not None:
            _lib.mtsv_index_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """Owning handle of an mtsv_batch (HBM-resident read batch + workspace)."""

    def __init__(self, index, device, max_reads, max_bases, max_hits_ws=0, lanes=0):
        self.index = index
        self.h = C.c_void_p()
        _check(lib().mtsv_batch_create_lanes(index.h, device, max_reads, max_bases, max_hits_ws, lanes,
                                             C.byref(self.h)))

    def reserve_host(self, n_reads, n_bases, warm_read_len=0):
        """mtsv_batch_reserve_host: size what run_host would size on its first calls; warm_read_len > 0 also runs a
        small batch sampled from the index through every kernel"""
        _check(lib().mtsv_batch_reserve_host(self.h, n_reads, n_bases, warm_read_len))

    def upload(self, bases, read_off):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        _check(lib().mtsv_batch_upload(self.h, bases.ctypes.data, read_off.ctypes.data,
                                       len(read_off) - 1))

    def set_verify_mode(self, mode):
        _check(lib().mtsv_batch_set_verify_mode(self.h, mode))

    def run(self, params=None):
        params = params or default_params()
        _check(lib().mtsv_batch_run(self.h, C.byref(params)))

    def run_host(self, bases, read_off, params=None):
        """mtsv_batch_run_host: host buffers of any size, sliced and double-buffered on the device."""
        params = params or default_params()
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        _check(lib().mtsv_batch_run_host(self.h, bases.ctypes.data, read_off.ctypes.data, len(read_off) - 1,
                                         C.byref(params)))

    def run_host_parts(self, parts, params=None):
        """parts: [(bases u8 array, read_off u64 array), ...]; the reads are numbered through the parts in order"""
        params = params or default_params()
        keep = [(np.ascontiguousarray(b, dtype=np.uint8), np.ascontiguousarray(o, dtype=np.uint64)) for b, o in parts]
        k = len(keep)
        bp = (C.c_void_p * k)(*[b.ctypes.data for b, _ in keep])
        op = (C.c_void_p * k)(*[o.ctypes.data for _, o in keep])
        nr = (C.c_uint64 * k)(*[len(o) - 1 for _, o in keep])
        _check(lib().mtsv_batch_run_host_parts(self.h, k, bp, op, nr, C.byref(params)))

    def stats(self):
        s = BatchStats()
        _check(lib().mtsv_batch_stats_get(self.h, C.byref(s)))
        return s.as_dict()

    def download(self):
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().mtsv_batch_download(self.h, C.byref(out), C.byref(n)))
        return _hits_from(out, n.value)

    def set_taxa_report(self, on):
        """mtsv_batch_set_taxa_report: every run from now on adds its reads to the workspace's per-TaxID counts"""
        _check(lib().mtsv_batch_set_taxa_report(self.h, int(bool(on))))

    def taxa_report(self, reset=False):
        """(rows as a TAXON_STATS_DTYPE array ascending by tax_id, total_reads, device_ms)"""
        out, n, total, ms = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_batch_taxa_report(self.h, C.byref(out), C.byref(n), C.byref(total), C.byref(ms), int(bool(reset))))
        return _taxon_rows_from(out, n.value), total.value, ms.value

    def set_match_flags(self, mode):
        """mtsv_batch_set_match_flags: MATCH_OFF, MATCH_WITH_HITS (hits and flags) or MATCH_ONLY (flags, no hits)"""
        _check(lib().mtsv_batch_set_match_flags(self.h, int(mode)))

    def match_flags(self):
        """(bool array with one entry per read of the last run: the run returned a hit for it, n_matched)"""
        out, n, m = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(lib().mtsv_batch_match_flags(self.h, C.byref(out), C.byref(n), C.byref(m)))
        try:
            nw = max((n.value + 63) // 64, 1)
            words = np.frombuffer((C.c_ubyte * (nw * 8)).from_address(out.value), dtype="<u8").copy()
        finally:
            lib().mtsv_free(out)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
        if bits[n.value:].any():
            raise MtsvError(E_DEVICE, "match flags set beyond the run's reads")
        return bits[:n.value], m.value

    def set_assignments(self, mode):
        """mtsv_batch_set_assignments: ASSIGN_OFF, ASSIGN_WITH_HITS (hits and assignments) or ASSIGN_ONLY (the hits stay
        on the device: download() returns none)"""
        _check(lib().mtsv_batch_set_assignments(self.h, int(mode)))

    def download_assignments(self):
        """(the last run's assignments as an ASSIGN_DTYPE array -- per read one record per distinct TaxID with the smallest
        edit, ascending by TaxID --, device ms of the collapse kernels)"""
        out, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_batch_download_assignments(self.h, C.byref(out), C.byref(n), C.byref(ms)))
        try:
            if n.value == 0:
                return np.zeros(0, dtype=ASSIGN_DTYPE), ms.value
            raw = (C.c_ubyte * (n.value * ASSIGN_DTYPE.itemsize)).from_address(out.value)
            return np.frombuffer(raw, dtype=ASSIGN_DTYPE).copy(), ms.value
        finally:
            lib().mtsv_free(out)

    def set_assignment_grain(self, grain):
        """mtsv_batch_set_assignment_grain: GRAIN_TAXID (16-byte records, download_assignments), GRAIN_TAXID_GI or
        GRAIN_LONG (24-byte records, download_assignments_gi); only while the assignments are ASSIGN_OFF"""
        _check(lib().mtsv_batch_set_assignment_grain(self.h, int(grain)))

    def download_assignments_gi(self):
        """(the last run's assignments as an ASSIGN_GI_DTYPE array -- per read one record per distinct (TaxID, GI, offset)
        with the smallest edit (GRAIN_LONG) or per distinct (TaxID, GI) with the smallest (edit, offset) (GRAIN_TAXID_GI),
        ascending --, device ms of the collapse kernels)"""
        out, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_batch_download_assignments_gi(self.h, C.byref(out), C.byref(n), C.byref(ms)))
        try:
            if n.value == 0:
                return np.zeros(0, dtype=ASSIGN_GI_DTYPE), ms.value
            raw = (C.c_ubyte * (n.value * ASSIGN_GI_DTYPE.itemsize)).from_address(out.value)
            return np.frombuffer(raw, dtype=ASSIGN_GI_DTYPE).copy(), ms.value
        finally:
            lib().mtsv_free(out)

    def format_text(self, read_ids):
        """mtsv_batch_format_text: (the result lines of the last run's assignments as bytes, written on the device; device ms).
        read_ids: the IDs of the reads the records number -- a list of str, or a (bytes, offsets) table"""
        return _format_text(lib().mtsv_batch_format_text, self.h, read_ids)

    def take_reads(self, src, keep=KEEP_UNMATCHED):
        """mtsv_batch_take_reads: this workspace's resident batch := the reads of src's last run whose match flag is clear
        (KEEP_MATCHED: set), handed over on the device; returns (n_kept, bases_kept, device ms of the kernels)"""
        n, nb, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_batch_take_reads(self.h, src.h, int(keep), C.byref(n), C.byref(nb), C.byref(ms)))
        return n.value, nb.value, ms.value

    def copy_reads(self, src):
        """mtsv_batch_copy_reads: this workspace's resident batch := a copy of src's (codes, offsets, read map), device to
        device; returns the device ms of the copies"""
        ms = C.c_float()
        _check(lib().mtsv_batch_copy_reads(self.h, src.h, C.byref(ms)))
        return ms.value

    def place_hits(self, hits=None):
        """mtsv_batch_place_hits: the alignments of the last run's hits, where they lie on the device (hits None), or of the
        given HIT_DTYPE hits against the resident batch.  Returns (placements as a PLACEMENT_DTYPE array, one per hit in the
        hits' order; the ops as a uint32 array, len << 4 | code, placement k owning ops[ops_off : ops_off + n_ops]; device ms)"""
        out, n, ops, n_ops, ms = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(), C.c_float()
        if hits is None:
            ptr, cnt = None, 0
        else:
            hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
            ptr, cnt = hits.ctypes.data, len(hits)
        _check(lib().mtsv_batch_place_hits(self.h, ptr, cnt, C.byref(out), C.byref(n), C.byref(ops), C.byref(n_ops), C.byref(ms)))
        try:
            pl = np.frombuffer((C.c_ubyte * (n.value * PLACEMENT_DTYPE.itemsize)).from_address(out.value), dtype=PLACEMENT_DTYPE).copy() \
                if n.value else np.zeros(0, dtype=PLACEMENT_DTYPE)
            op = np.frombuffer((C.c_ubyte * (n_ops.value * 4)).from_address(ops.value), dtype="<u4").copy() \
                if n_ops.value else np.zeros(0, dtype="<u4")
            return pl, op, ms.value
        finally:
            lib().mtsv_free(out)
            lib().mtsv_free(ops)

    def merge_runs(self, srcs):
        """mtsv_batch_merge_runs: the last runs of srcs (the same reads in each) merged per read into this workspace, in
        source order; download(), stats(), match_flags() and taxa_report() then speak of the merge.  Returns the device
        ms of the merge kernels"""
        srcs = list(srcs)
        arr = (C.c_void_p * max(len(srcs), 1))(*[s.h for s in srcs])
        ms = C.c_float()
        _check(lib().mtsv_batch_merge_runs(self.h, arr, len(srcs), C.byref(ms)))
        return ms.value

    def take_unique(self, src, dupmap):
        """mtsv_batch_take_unique: this workspace's resident batch := the first read of every group of identical reads of
        src's resident batch, handed over on the device; dupmap (a DupMap) then holds the groups.  Returns (n_unique,
        bases_kept, device ms of the kernels)"""
        n, nb, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_batch_take_unique(self.h, src.h, dupmap.h, C.byref(n), C.byref(nb), C.byref(ms)))
        return n.value, nb.value, ms.value

    def read_map(self):
        """the caller's read number of every resident read (uint64 array; the identity after upload)"""
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().mtsv_batch_read_map(self.h, C.byref(out), C.byref(n)))
        try:
            return np.frombuffer((C.c_ubyte * (max(n.value, 1) * 8)).from_address(out.value), dtype="<u8")[:n.value].copy()
        finally:
            lib().mtsv_free(out)

    def download_reads(self):
        """(codes uint8 0..4, read_off uint64 with n + 1 entries): the resident batch as the kernels see it (tests)"""
        codes, off, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(lib().mtsv_batch_download_reads(self.h, C.byref(codes), C.byref(off), C.byref(n)))
        try:
            o = np.frombuffer((C.c_ubyte * ((n.value + 1) * 8)).from_address(off.value), dtype="<u8").copy()
            nb = int(o[-1])
            c = np.frombuffer((C.c_ubyte * max(nb, 1)).from_address(codes.value), dtype=np.uint8)[:nb].copy()
        finally:
            lib().mtsv_free(codes)
            lib().mtsv_free(off)
        return c, o

    def close(self):
        if self.h is not None and _lib is not None:
            _lib.mtsv_batch_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _id_table(read_ids):
    """(blob, id_off) as mtsv_format_assignments takes them: from a list of IDs, the NUL-terminated IDs back to back, as
    format_assignments builds them; a (bytes, offsets) pair is a table already and passes through (its slots may be NUL-padded
    or filled to the last byte)"""
    if isinstance(read_ids, tuple):
        blob, off = read_ids
        return bytes(blob), np.ascontiguousarray(off, dtype=np.uint64)
    blob = b"".join(i.encode() + b"\0" for i in read_ids)
    off = np.zeros(len(read_ids) + 1, dtype=np.uint64)
    np.cumsum([len(i.encode()) + 1 for i in read_ids], out=off[1:])
    return blob, off


def _format_text(call, handle, read_ids):
    blob, off = _id_table(read_ids)
    out, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
    _check(call(handle, blob, off.ctypes.data, len(off) - 1, C.byref(out), C.byref(n), C.byref(ms)))
    try:
        if C.string_at(out.value + n.value, 1) != b"\0":
            raise MtsvError(E_DEVICE, "the text does not end with a NUL")
        return C.string_at(out.value, n.value), ms.value
    finally:
        lib().mtsv_free(out)


def _records_from(ptr, n, dtype):
    try:
        if n == 0:
            return np.zeros(0, dtype=dtype)
        raw = (C.c_ubyte * (n * dtype.itemsize)).from_address(ptr.value)
        return np.frombuffer(raw, dtype=dtype).copy()
    finally:
        lib().mtsv_free(ptr)


class Fold:
    """Owning handle of an mtsv_fold: assignment records of one grain accumulated in HBM across runs -- the sorted union
    of everything folded so far, one record per key with the better value.  Bound to a device and a grain, not to an
    index: the workspaces and indexes whose runs it took may be closed."""

    def __init__(self, device=0, grain=GRAIN_TAXID, n_reads=None):
        self.grain = int(grain)
        self.h = C.c_void_p()
        _check(lib().mtsv_fold_create(device, self.grain, C.byref(self.h)))
        if n_reads is not None:
            self.reset(n_reads)

    def reset(self, n_reads):
        """mtsv_fold_reset: empty, for reads numbered below n_reads, TaxID union cleared"""
        _check(lib().mtsv_fold_reset(self.h, int(n_reads)))

    def add_run(self, src):
        """mtsv_fold_add_run: folds the assignments of the last run of the Batch src; returns the device ms of the fold"""
        ms = C.c_float()
        _check(lib().mtsv_fold_add_run(self.h, src.h, C.byref(ms)))
        return ms.value

    def add_records(self, records):
        """mtsv_fold_add_records: folds host records (ASSIGN_DTYPE, or ASSIGN_GI_DTYPE in the wide grains), keys strictly
        ascending; returns the device ms of the fold"""
        dt = ASSIGN_DTYPE if self.grain == GRAIN_TAXID else ASSIGN_GI_DTYPE
        records = np.ascontiguousarray(records, dtype=dt)
        ms = C.c_float()
        _check(lib().mtsv_fold_add_records(self.h, records.ctypes.data, len(records), C.byref(ms)))
        return ms.value

    def add_text(self, hits, line_off, line_read):
        """mtsv_fold_add_text: parses the hit parts of result lines on the device and folds their records.  hits: bytes (or a
        uint8 array), line_off: n_lines + 1 offsets into it, line_read: the lines' read numbers; returns (tokens, records,
        device ms)"""
        hits = np.frombuffer(hits, dtype=np.uint8) if isinstance(hits, (bytes, bytearray)) else np.ascontiguousarray(hits, dtype=np.uint8)
        line_off = np.ascontiguousarray(line_off, dtype=np.uint64)
        line_read = np.ascontiguousarray(line_read, dtype=np.uint32)
        n_lines = len(line_read)
        if n_lines and len(line_off) != n_lines + 1:
            raise ValueError("line_off must hold one more entry than line_read")
        n_tok, n_rec, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_fold_add_text(self.h, hits.ctypes.data if len(hits) else None, line_off.ctypes.data if n_lines else None,
                                        line_read.ctypes.data if n_lines else None, n_lines, C.byref(n_tok), C.byref(n_rec), C.byref(ms)))
        return n_tok.value, n_rec.value, ms.value

    def count(self):
        n = C.c_uint64()
        _check(lib().mtsv_fold_count(self.h, C.byref(n)))
        return n.value

    def download(self):
        """the accumulated records as an ASSIGN_DTYPE array (GRAIN_TAXID)"""
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().mtsv_fold_download(self.h, C.byref(out), C.byref(n)))
        return _records_from(out, n.value, ASSIGN_DTYPE)

    def download_gi(self):
        """the accumulated records as an ASSIGN_GI_DTYPE array (GRAIN_TAXID_GI, GRAIN_LONG)"""
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().mtsv_fold_download_gi(self.h, C.byref(out), C.byref(n)))
        return _records_from(out, n.value, ASSIGN_GI_DTYPE)

    def taxa_report(self):
        """(rows as a TAXON_STATS_DTYPE array ascending by tax_id, total_reads, device_ms) of the accumulated records"""
        out, n, total, ms = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_fold_taxa_report(self.h, C.byref(out), C.byref(n), C.byref(total), C.byref(ms)))
        return _taxon_rows_from(out, n.value), total.value, ms.value

    def match_flags(self):
        """(bool array over the n_reads of reset: the read has a record, n_matched)"""
        out, n, m = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(lib().mtsv_fold_match_flags(self.h, C.byref(out), C.byref(n), C.byref(m)))
        try:
            nw = max((n.value + 63) // 64, 1)
            words = np.frombuffer((C.c_ubyte * (nw * 8)).from_address(out.value), dtype="<u8").copy()
        finally:
            lib().mtsv_free(out)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
        if bits[n.value:].any():
            raise MtsvError(E_DEVICE, "match flags set beyond the fold's reads")
        return bits[:n.value], m.value

    def format_text(self, read_ids):
        """mtsv_fold_format_text: (the result lines of the accumulated records as bytes, written on the device; device ms).
        read_ids: the IDs of the n_reads reads of reset -- a list of str, or a (bytes, offsets) table"""
        return _format_text(lib().mtsv_fold_format_text, self.h, read_ids)

    def lca(self, tx, slack=0, out=None, rows=True):
        """mtsv_fold_lca: per read with a record the LCA, in the Taxonomy tx, of its TaxIDs within `slack` edits of its
        smallest edit (SLACK_ALL: all of them).  out: another Fold of this device at GRAIN_TAXID that takes one record
        (read, LCA, smallest edit) per read.  Returns (clade rows as a CLADE_STATS_DTYPE array in preorder, or None without
        rows; total_reads; device ms)"""
        ptr, n, total, ms = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_fold_lca(self.h, tx.h, int(slack), out.h if out is not None else None, C.byref(ptr) if rows else None,
                                   C.byref(n), C.byref(total), C.byref(ms)))
        return (_records_from(ptr, n.value, CLADE_STATS_DTYPE) if rows else None), total.value, ms.value

    def abundance(self, weights, slack=SLACK_ALL, max_iters=100, tol=0, out=None, rows=True):
        """mtsv_fold_abundance: expectation-maximisation over the reads' entering taxa (those within `slack` edits of the read's
        smallest; SLACK_ALL: all).  weights: the table of abundance_weights, 1 .. 255 uint32 in units of 2^-32; tol: the L1
        change, in units of 2^-32 reads, at which the loop stops.  out: another Fold of this device at GRAIN_TAXID that takes
        one record (read, assigned TaxID, its smallest edit) per read.  Returns (rows as an ABUNDANCE_ROW_DTYPE array ascending
        by tax_id, or None without rows; the info as a dict; device ms)"""
        w = np.ascontiguousarray(weights, dtype="<u4")
        ptr, n, info, ms = C.c_void_p(), C.c_uint64(), AbundanceInfo(), C.c_float()
        _check(lib().mtsv_fold_abundance(self.h, w.ctypes.data, len(w), int(slack), int(max_iters), int(tol), out.h if out is not None else None,
                                         C.byref(ptr) if rows else None, C.byref(n), C.byref(info), C.byref(ms)))
        return (_records_from(ptr, n.value, ABUNDANCE_ROW_DTYPE) if rows else None), info.as_dict(), ms.value

    def pair(self, mode, max_insert=0, unpaired_edits=0, out=None):
        """mtsv_fold_pair: reads 2p and 2p + 1 of this fold are the mates of pair p; the Fold out (this device, GRAIN_TAXID)
        becomes the fold of the pairs: one record (p, TaxID, edit) per TaxID that PAIR_BOTH, PAIR_EITHER or PAIR_PROPER keeps.
        Returns (stats as a dict, device ms)"""
        st, ms = PairStats(), C.c_float()
        _check(lib().mtsv_fold_pair(self.h, int(mode), int(max_insert), int(unpaired_edits), out.h if out is not None else None,
                                    C.byref(st), C.byref(ms)))
        return st.as_dict(), ms.value

    def expand(self, src, dupmap):
        """mtsv_fold_expand: this fold := for every read of dupmap's last take the records the Fold src holds for the read's
        representative, numbered as that read; returns the device ms of the kernels"""
        ms = C.c_float()
        _check(lib().mtsv_fold_expand(self.h, src.h, dupmap.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h is not None and _lib is not None:
            _lib.mtsv_fold_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DupMap:
    """Owning handle of an mtsv_dupmap: which reads of the last Batch.take_unique are identical.  MTSV_DEDUP_HASH_BITS and
    MTSV_FAN_TILE are read when it is created."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _check(lib().mtsv_dupmap_create(device, C.byref(self.h)))

    def download(self):
        """(read, rep, n_unique): per resident read of the take's source the caller's number of the read and of the first
        read identical to it, as uint64 arrays; empty before any take"""
        a, b, n, u = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(lib().mtsv_dupmap_download(self.h, C.byref(a), C.byref(b), C.byref(n), C.byref(u)))
        try:
            nbytes = max(n.value, 1) * 8
            read = np.frombuffer((C.c_ubyte * nbytes).from_address(a.value), dtype="<u8")[:n.value].copy()
            rep = np.frombuffer((C.c_ubyte * nbytes).from_address(b.value), dtype="<u8")[:n.value].copy()
        finally:
            lib().mtsv_free(a)
            lib().mtsv_free(b)
        return read, rep, u.value

    def close(self):
        if self.h is not None and _lib is not None:
            _lib.mtsv_dupmap_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Coverage:
    """Owning handle of an mtsv_coverage: per reference sequence (tax_id, gi) the reads, alignments, aligned bases and covered
    bases of the GRAIN_LONG folds it is given.  Bound to a device.  MTSV_COVER_TILE, MTSV_COVER_LANE_MAX, MTSV_TRACE and
    MTSV_COVER_TIMING are read when it is created."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _check(lib().mtsv_coverage_create(device, C.byref(self.h)))

    def add_index(self, index):
        """mtsv_coverage_add_index: the bins of an MGIndex join the table (host only)"""
        _check(lib().mtsv_coverage_add_index(self.h, index.h))

    def add_refs(self, tax_id, gi, length):
        """mtsv_coverage_add_refs: references from three arrays of equal length"""
        tax_id = np.ascontiguousarray(tax_id, dtype=np.uint32)
        gi = np.ascontiguousarray(gi, dtype=np.uint32)
        length = np.ascontiguousarray(length, dtype=np.uint64)
        if not len(tax_id) == len(gi) == len(length):
            raise ValueError("tax_id, gi and length must be of one length")
        _check(lib().mtsv_coverage_add_refs(self.h, tax_id.ctypes.data, gi.ctypes.data, length.ctypes.data, len(tax_id)))

    def reset(self):
        """mtsv_coverage_reset: counters and bitmap zero; the table stays"""
        _check(lib().mtsv_coverage_reset(self.h))

    def add_fold(self, fold, read_len, slack=0):
        """mtsv_coverage_add_fold: the records of the Fold (GRAIN_LONG) within `slack` edits of their read's smallest edit
        (SLACK_ALL: all of them) are added; read_len: the lengths of the fold's n_reads reads; returns the device ms"""
        read_len = np.ascontiguousarray(read_len, dtype=np.uint32)
        ms = C.c_float()
        _check(lib().mtsv_coverage_add_fold(self.h, fold.h, read_len.ctypes.data, len(read_len), int(slack), C.byref(ms)))
        return ms.value

    def rows(self):
        """(every reference of the table as a REF_COVERAGE_DTYPE array ascending by (tax_id, gi), device ms)"""
        out, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_coverage_rows(self.h, C.byref(out), C.byref(n), C.byref(ms)))
        return _records_from(out, n.value, REF_COVERAGE_DTYPE), ms.value

    def close(self):
        if self.h is not None and _lib is not None:
            _lib.mtsv_coverage_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_coverage_report(rows):
    """mtsv_format_coverage_report: the TSV of mtsv-binner --coverage, as bytes"""
    out_rows = np.zeros(len(rows), dtype=REF_COVERAGE_DTYPE)
    for f in REF_COVERAGE_DTYPE.names:
        out_rows[f] = rows[f]
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_coverage_report(out_rows.ctypes.data, len(out_rows), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib().mtsv_free(out)


class Pileup:
    """Owning handle of an mtsv_pileup: per reference position the counters match, A, C, G, T, N, del, ins of the placed hits it
    is given.  Bound to a device and to a list of TaxIDs (None or empty: every reference).  MTSV_PILE_TILE, MTSV_TRACE and
    MTSV_PILE_TIMING are read when it is created."""

    def __init__(self, device=0, taxa=None):
        self.h = C.c_void_p()
        t = np.ascontiguousarray([] if taxa is None else list(taxa), dtype=np.uint32)
        _check(lib().mtsv_pileup_create(device, t.ctypes.data if len(t) else None, len(t), C.byref(self.h)))

    def reset(self):
        """mtsv_pileup_reset: counters zero, the references stay"""
        _check(lib().mtsv_pileup_reset(self.h))

    def add_run(self, batch, hits=None, slack=0):
        """mtsv_pileup_add_run: the hits of the Batch's last run where they lie (hits None), or the given HIT_DTYPE hits against
        its resident batch, within `slack` edits of their read's smallest edit in this call (SLACK_ALL: all of them);
        returns (hits piled, hits skipped, device ms)"""
        piled, skipped, ms = C.c_uint64(), C.c_uint64(), C.c_float()
        if hits is None:
            ptr, cnt = None, 0
        else:
            hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
            ptr, cnt = hits.ctypes.data, len(hits)
        _check(lib().mtsv_pileup_add_run(self.h, batch.h, ptr, cnt, int(slack), C.byref(piled), C.byref(skipped), C.byref(ms)))
        return piled.value, skipped.value, ms.value

    def info(self):
        """mtsv_pileup_info as a dict"""
        out = PileupInfo()
        _check(lib().mtsv_pileup_info(self.h, C.byref(out)))
        return out.as_dict()

    def download(self, tax_id, gi):
        """(the reference's counters as a uint32 array [slot][8], channel 0 integrated; its ref codes, uint8 per slot)"""
        cnt, ref, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(lib().mtsv_pileup_download(self.h, int(tax_id), int(gi), C.byref(cnt), C.byref(ref), C.byref(n)))
        try:
            counts = np.frombuffer((C.c_ubyte * (n.value * 32)).from_address(cnt.value), dtype="<u4").reshape(n.value, 8).copy()
            codes = np.frombuffer((C.c_ubyte * n.value).from_address(ref.value), dtype=np.uint8).copy()
            return counts, codes
        finally:
            lib().mtsv_free(cnt)
            lib().mtsv_free(ref)

    def sites(self, min_depth=0, min_alt=0, min_alt_ppm=0):
        """mtsv_pileup_sites: (the sites as a PILE_SITE_DTYPE array ascending by (tax_id, gi, pos), device ms)"""
        out, n, ms = C.c_void_p(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_pileup_sites(self.h, int(min_depth), int(min_alt), int(min_alt_ppm), C.byref(out), C.byref(n), C.byref(ms)))
        return _records_from(out, n.value, PILE_SITE_DTYPE), ms.value

    def consensus(self, min_depth=1, min_frac_ppm=500000, min_breadth_ppm=0, fill=CONS_FILL_N, line_width=60, fasta=True):
        """mtsv_pileup_consensus: (the FASTA text as bytes, or None with fasta=False; the emitted references' rows as a
        CONS_REF_DTYPE array ascending by (tax_id, gi); device ms)"""
        text, n_text, out, n, ms = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(), C.c_float()
        _check(lib().mtsv_pileup_consensus(self.h, int(min_depth), int(min_frac_ppm), int(min_breadth_ppm), int(fill), int(line_width),
                                           C.byref(text) if fasta else None, C.byref(n_text) if fasta else None, C.byref(out), C.byref(n), C.byref(ms)))
        rows = _records_from(out, n.value, CONS_REF_DTYPE)
        if not fasta:
            return None, rows, ms.value
        try:
            return C.string_at(text.value, n_text.value), rows, ms.value
        finally:
            lib().mtsv_free(text)

    def add_counts(self, tax_id, gi, first_slot, counts, n_hits):
        """mtsv_pileup_add_counts: counts [n_slots][8] uint32, plain as download gives them, added to the reference's slots from
        first_slot; n_hits is added to hits_piled"""
        c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1, 8)
        _check(lib().mtsv_pileup_add_counts(self.h, int(tax_id), int(gi), int(first_slot), len(c), c.ctypes.data if len(c) else None, int(n_hits)))

    def close(self):
        if self.h is not None and _lib is not None:
            _lib.mtsv_pileup_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_variants(rows):
    """mtsv_format_variants: the TSV of mtsv-binner --variants, as one str"""
    r = np.ascontiguousarray(rows, dtype=PILE_SITE_DTYPE)
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_variants(r.ctypes.data, len(r), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value).decode()
    finally:
        lib().mtsv_free(out)


def format_consensus_stats(rows):
    """mtsv_format_consensus_stats: the TSV of mtsv-binner --consensus-stats, as one str"""
    r = np.ascontiguousarray(rows, dtype=CONS_REF_DTYPE)
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_consensus_stats(r.ctypes.data if len(r) else None, len(r), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value).decode()
    finally:
        lib().mtsv_free(out)


class Taxonomy:
    """Owning handle of an mtsv_taxonomy: an NCBI nodes.dmp as a tree on the host (no device needed)"""

    def __init__(self, path):
        self.h = C.c_void_p()
        _check(lib().mtsv_taxonomy_load(os.fsencode(path), C.byref(self.h)))

    def info(self):
        """{n_nodes, n_implied_roots, n_ranks, max_depth}"""
        i = TaxonomyInfo()
        _check(lib().mtsv_taxonomy_info(self.h, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in TaxonomyInfo._fields_}

    def parent(self, tax_id):
        """(the parent's TaxID, the rank code) of a TaxID; (0, RANK_UNKNOWN) for one the file does not know"""
        p, r = C.c_uint32(), C.c_uint32()
        _check(lib().mtsv_taxonomy_parent(self.h, int(tax_id), C.byref(p), C.byref(r)))
        return p.value, r.value

    def rank_name(self, rank):
        return lib().mtsv_taxonomy_rank_name(self.h, int(rank)).decode()

    def close(self):
        if self.h is not None and _lib is not None:
            _lib.mtsv_taxonomy_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def abundance_weights(q, n_w=64):
    """mtsv_abundance_weights: w[d - 1] = min(floor(q^d * 2^32), 2^32 - 1) for d = 1 .. n_w, as a uint32 array; 0 < q <= 1"""
    w = np.zeros(max(int(n_w), 1), dtype="<u4")
    _check(lib().mtsv_abundance_weights(float(q), int(n_w), w.ctypes.data))
    return w[:int(n_w)]


def format_abundance(rows, info):
    """mtsv_format_abundance: the TSV of mtsv-collapse --abundance, as bytes; info: the dict of Fold.abundance (total_mass is used)"""
    out_rows = np.zeros(len(rows), dtype=ABUNDANCE_ROW_DTYPE)
    for f in ABUNDANCE_ROW_DTYPE.names:
        out_rows[f] = rows[f]
    c_info = AbundanceInfo(**{k: int(v) for k, v in info.items()})
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_abundance(out_rows.ctypes.data, len(out_rows), C.byref(c_info), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib().mtsv_free(out)


def format_clade_report(rows, total_reads, tx=None):
    """mtsv_format_clade_report: the TSV of mtsv-collapse --clade-report, as bytes; without tx every rank is '-'"""
    out_rows = np.zeros(len(rows), dtype=CLADE_STATS_DTYPE)
    for f in CLADE_STATS_DTYPE.names:
        out_rows[f] = rows[f]
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_clade_report(out_rows.ctypes.data, len(out_rows), int(total_reads), tx.h if tx is not None else None,
                                          C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib().mtsv_free(out)


def format_results(hits, read_ids, long_format=False):
    """write_assignments over a batch: returns the result lines as one str."""
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    blob = b"".join(i.encode() + b"\0" for i in read_ids)
    off = np.zeros(len(read_ids) + 1, dtype=np.uint64)
    np.cumsum([len(i.encode()) + 1 for i in read_ids], out=off[1:])
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_results(hits.ctypes.data, len(hits), blob, off.ctypes.data,
                                     len(read_ids), int(long_format), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value).decode()
    finally:
        lib().mtsv_free(out)


def format_assignments(a, read_ids):
    """mtsv_format_assignments: the short-format result lines from assignments, as one str"""
    a = np.ascontiguousarray(a, dtype=ASSIGN_DTYPE)
    blob = b"".join(i.encode() + b"\0" for i in read_ids)
    off = np.zeros(len(read_ids) + 1, dtype=np.uint64)
    np.cumsum([len(i.encode()) + 1 for i in read_ids], out=off[1:])
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_assignments(a.ctypes.data, len(a), blob, off.ctypes.data, len(read_ids), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value).decode()
    finally:
        lib().mtsv_free(out)


def format_placements(placements, ops, read_ids):
    """mtsv_format_placements: one line READ_ID TAXID GI +|- START END EDIT CIGAR (tab-separated) per placement, as one str"""
    pl = np.ascontiguousarray(placements, dtype=PLACEMENT_DTYPE)
    ops = np.ascontiguousarray(ops, dtype="<u4")
    blob = b"".join(i.encode() + b"\0" for i in read_ids)
    off = np.zeros(len(read_ids) + 1, dtype=np.uint64)
    np.cumsum([len(i.encode()) + 1 for i in read_ids], out=off[1:])
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_placements(pl.ctypes.data, len(pl), ops.ctypes.data, blob, off.ctypes.data, len(read_ids), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value).decode()
    finally:
        lib().mtsv_free(out)


def format_assignments_gi(a, read_ids):
    """mtsv_format_assignments_gi: the long-format result lines (READ_ID:TAX-GI-OFFSET=EDIT,...) from wide assignments,
    as one str"""
    a = np.ascontiguousarray(a, dtype=ASSIGN_GI_DTYPE)
    blob = b"".join(i.encode() + b"\0" for i in read_ids)
    off = np.zeros(len(read_ids) + 1, dtype=np.uint64)
    np.cumsum([len(i.encode()) + 1 for i in read_ids], out=off[1:])
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_assignments_gi(a.ctypes.data, len(a), blob, off.ctypes.data, len(read_ids), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value).decode()
    finally:
        lib().mtsv_free(out)


def _taxon_rows_from(ptr, n):
    try:
        if n == 0:
            return np.zeros(0, dtype=TAXON_STATS_DTYPE)
        raw = (C.c_ubyte * (n * TAXON_STATS_DTYPE.itemsize)).from_address(ptr.value)
        return np.frombuffer(raw, dtype=TAXON_STATS_DTYPE).copy()
    finally:
        lib().mtsv_free(ptr)


def _taxon_rows(rows):
    # (field by field: an array of another layout, or a zeroed one, must not carry its padding over)
    out = np.zeros(len(rows), dtype=TAXON_STATS_DTYPE)
    for f in TAXON_STATS_DTYPE.names:
        out[f] = rows[f]
    return out


def merge_taxa_reports(a, b):
    """mtsv_merge_taxa_reports: the rows of two workspaces that shared one input, summed per TaxID"""
    a, b = _taxon_rows(a), _taxon_rows(b)
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_merge_taxa_reports(a.ctypes.data, len(a), b.ctypes.data, len(b), C.byref(out), C.byref(n)))
    return _taxon_rows_from(out, n.value)


def format_taxa_report(rows, total_reads):
    """write_taxa_report: the TSV of mtsv-collapse --report, as bytes"""
    rows = _taxon_rows(rows)
    out, n = C.c_void_p(), C.c_uint64()
    _check(lib().mtsv_format_taxa_report(rows.ctypes.data, len(rows), int(total_reads), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out.value, n.value)
    finally:
        lib().mtsv_free(out)


def synth_reads(index, seed, n_reads, read_len):
    bases = np.empty(n_reads * read_len, dtype=np.uint8)
    off = np.empty(n_reads + 1, dtype=np.uint64)
    _check(lib().mtsv_synth_reads(index.h, seed, n_reads, read_len, bases.ctypes.data,
                                  off.ctypes.data))
    return bases, off
