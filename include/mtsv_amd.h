/*
 * mtsv_amd.h -- C ABI of the MI355X-native mtsv-binner hot path (libmtsv_amd.so).
 *
 * Plain C: opaque handles, pointers and sizes only.  A Rust host binds it the way the reference
 * already binds its only native dependency (extern "C" block + #[repr(C)] mirrors + RAII Drop:
 * ssw/src/lib.rs:108-154, :26-32); INTEGRATION.md shows the stub.
 *
 * Every int-returning function returns 0 on success and a negative MTSV_E_* code otherwise;
 * mtsv_last_error() returns a thread-local message.  There is NO CPU fallback: a call that needs
 * the GPU fails with MTSV_E_DEVICE when no gfx950 device / HIP runtime is usable.
 *
 * What each entry point replaces in the reference (paths relative to FofanovLab/mtsv_tools):
 *   mtsv_index_load        io::from_file::<MGIndex>                      src/io.rs:115-123, src/binner.rs:63
 *   mtsv_index_to_device   FMIndex::new(bwt, less, occ) (borrow -> HBM)  src/binner.rs:64-67
 *   mtsv_bin_batch         the worker closure: normalise, matching_tax_ids(fwd), revcomp,
 *                          matching_tax_ids(rev), chain                   src/binner.rs:77-131,
 *                          MGIndex::matching_tax_ids                      src/index.rs:258-432
 *   mtsv_hit               Hit {tax_id, gi, offset, edit}                 src/index.rs:30-40
 *   mtsv_params            matching_tax_ids' scalar arguments             src/index.rs:258-269
 *                          (defaults: src/bin/mtsv-binner.rs:63-94)
 *   mtsv_format_results    write_assignments                              src/binner.rs:310-379
 *   mtsv_batch_set_assignments, mtsv_batch_download_assignments, mtsv_format_assignments
 *                          its reduction, smallest edit per TaxID ascending,     src/binner.rs:355-378
 *                          on the device, and the default-format lines from that
 *   mtsv_index_build*, mtsv_index_write
 *                          MGIndex::new + io::write_to_file               src/index.rs:491-582, src/io.rs:125-133
 *   mtsv_batch_set_match_flags, mtsv_batch_match_flags
 *                          the set of read IDs mtsv-partition collects from      src/bin/mtsv-partition.rs:34-54
 *                          the results text, as one bit per read of a run
 *   mtsv_batch_*           the same path as mtsv_bin_batch, split so a host can keep read
 *                          batches resident in HBM and overlap upload / run / download
 *                          (replaces the bounded queue of vendor/cue/src/lib.rs:45-105)
 */
#ifndef MTSV_AMD_H
#define MTSV_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTSV_OK 0
#define MTSV_E_ARG (-1)      /* invalid argument */
#define MTSV_E_IO (-2)       /* file cannot be opened / read / written */
#define MTSV_E_FORMAT (-3)   /* MG-index bytes violate the bincode layout or its invariants */
#define MTSV_E_DEVICE (-4)   /* no usable HIP device, HIP error, or device-side capacity */
#define MTSV_E_LIMIT (-5)    /* input exceeds a documented limit of the device layout */
#define MTSV_E_NOMEM (-6)

typedef struct mtsv_index mtsv_index; /* host copy of the MG-index + per-device HBM layout */
typedef struct mtsv_batch mtsv_batch; /* device workspace for one batch of reads on one GPU */

/* scalar arguments of MGIndex::matching_tax_ids (src/index.rs:258-269) */
typedef struct {
    double edit_rate;        /* -e / --edit-rate      0.13  */
    uint32_t seed_size;      /* --seed-size           18    */
    uint32_t seed_interval;  /* --seed-interval       15    */
    double min_seed;         /* --min-seed            0.015 */
    uint64_t max_hits;       /* --max-hits            2000  */
    uint64_t tune_max_hits;  /* --tune-max-hits       200   */
    int64_t max_assignments; /* --max-assignments     -1 = None */
    int64_t max_candidates;  /* --max-candidates      -1 = None */
} mtsv_params;

/* one Hit (src/index.rs:30-40) tagged with the read it belongs to and the strand call
 * (0 = forward, binner.rs:102; 1 = reverse complement, binner.rs:116) that produced it */
typedef struct {
    uint64_t read;   /* index of the read inside the batch */
    uint32_t tax_id;
    uint32_t gi;
    uint32_t edit;
    uint8_t strand;
    uint8_t _pad[3];
    uint64_t offset; /* candidate start - bin start (index.rs:416) */
} mtsv_hit;

/* shape of a loaded index */
typedef struct {
    uint64_t n;        /* symbols in `sequences`, including the trailing '$' */
    uint64_t n_bins;   /* reference sequences (GI records) */
    uint32_t occ_k;    /* Occ sampling interval of the file */
    uint64_t sa_s;     /* suffix-array sampling interval of the file */
    uint64_t file_bytes;
    uint64_t device_bytes; /* HBM held on the device it was last uploaded to (0 if none) */
    uint32_t kmer_k;       /* symbols of the resident k-mer interval table on that device (0: none) */
    uint32_t sa_full;      /* 1 when the full suffix array is resident there */
} mtsv_index_info_t;

/* per-stage device time of the last mtsv_batch_run, measured with HIP events on the batch's
 * own stream, plus the work counters the roofline accounting needs */
#define MTSV_N_STAGES 8
typedef struct {
    float stage_ms[MTSV_N_STAGES]; /* search, thin+scan, expand, locate, coalesce, verify, gather, total */
    uint64_t n_reads;
    uint64_t n_seed_slots;  /* seeds searched (both strands) */
    uint64_t n_seed_hits;   /* located seed hits */
    uint64_t lf_steps;      /* LF steps walked by k_locate (0 when the full SA is resident) */
    uint64_t n_candidates;  /* candidates after coalescing + min_seeds filter */
    uint64_t n_verified;    /* candidates whose window went through the SW prefilter */
    uint64_t window_bytes;  /* summed window length of those */
    uint64_t n_hits;        /* hits returned */
    uint64_t n_passes;      /* >1 when the batch had to be split to fit the hit workspace */
    uint64_t n_rounds;      /* verification rounds of the last pass: 1 + rounds that took the successors of
                             * candidates that passed the SW prefilter and failed the edit distance */
    uint64_t n_lanes;       /* concurrent parts the batch ran as (MTSV_LANES, default 3 for >= 98304 reads): with
                             * more than one, stage_ms[0..6] are device times summed over the overlapping parts
                             * and stage_ms[7] is the wall time of the run */
    uint64_t sw_cell_pairs; /* k_sw_pairs: DP cell pairs its sweeps computed, per 16-lane group (one packed
                             * 7-instruction recurrence each; 4 groups share a wave instruction) */
    float sw_prefilter_ms;  /* device time of the SW prefilter's kernels in the first round of every pass (HIP events on
                             * the lane's stream), summed over lanes like stage_ms; part of stage_ms[5] */
    float sw_sweep_ms;      /* of that, the DP sweeps (k_sw_pairs); the rest of sw_prefilter_ms is sw_diag_ms + sw_bound_ms */
    uint64_t n_sw_passed;   /* candidates whose SW score reached the threshold of index.rs:406, i.e. the edit
                             * distances the reference computes (:407-409).  Counted where the prefilter is a
                             * kernel of its own (reference order, reads up to 253 bases); 0 otherwise */
    float sw_diag_ms;       /* k_sw_diag: the lower bounds on the seed diagonal */
    float sw_bound_ms;      /* k_edit_myers in fused mode (bound + edit distance of round 0; sw_diag_ms is 0 then), or in bound mode
                               (MTSV_SW_FUSED=0): the two-sided bound by the unit-cost edit distance */
    float edit_ms;          /* k_edit_myers on the candidates that passed the prefilter (first round of every pass) */
    uint64_t myers_columns; /* window columns the bit-vector recurrences of k_edit_myers advanced (bound + edit distance) */
    uint64_t n_sw_bound_refuted; /* candidates the edit-distance bound refuted without a sweep */
    uint64_t verify_turns;     /* passes that took the workspace's verify turn (0: one lane, or MTSV_VERIFY_TURN=0) */
    uint64_t verify_lanes_max; /* lanes that had the verify kernels of a pass in flight at once, at most (1 with the turn) */
    uint64_t myers_grid_max;   /* largest k_edit_myers grid of the run, in workgroups (at most 256 x MTSV_MYERS_WGS_PER_CU) */
    uint64_t n_seed_tile_passes; /* of n_passes, those whose seed stage ran by tiles (k_thin_tiled, k_expand_tiled); the others
                                  * (MTSV_SEED_STAGE=legacy, or a pass that does not fit the tile) ran k_thin and k_expand */
} mtsv_batch_stats;

const char *mtsv_last_error(void);
const char *mtsv_version(void);
void mtsv_params_default(mtsv_params *p);

/* number of visible HIP devices (0 when none / no runtime); never fails */
int mtsv_device_count(void);

/* ---- MG-index: load / build / write ----------------------------------------------------- */
int mtsv_index_load(const char *path, mtsv_index **out);
/* MGIndex::new: entries in database insertion order; sorted by tax_id (stable) like the BTreeMap */
int mtsv_index_build(uint64_t n_seqs, const uint32_t *tax_ids, const uint32_t *gis,
                     const uint8_t *const *seqs, const uint64_t *seq_lens, uint32_t occ_k,
                     uint64_t sa_s, int n_threads, mtsv_index **out);
/* mtsv-build: FASTA with `SEQID-TAXID` headers (src/util.rs:26-56, src/io.rs:135-150) */
int mtsv_index_build_fasta(const char *fasta_path, uint32_t occ_k, uint64_t sa_s, int n_threads,
                           mtsv_index **out);
/* Where later mtsv_index_build* / mtsv_synth_index calls run the suffix sort: a HIP device ordinal (prefix
 * doubling in HBM, ~32 B per symbol) or -1 = host threads (default).  The index bytes are the same. */
int mtsv_set_build_device(int hip_device);
int mtsv_index_write(const mtsv_index *ix, const char *path);
int mtsv_index_info(const mtsv_index *ix, mtsv_index_info_t *info);
void mtsv_index_free(mtsv_index *ix);

/* Re-pack the FM-index into the HBM layout of DESIGN.md and upload it to `hip_device`.
 * flags: MTSV_DEV_* below.  Idempotent per device. */
#define MTSV_DEV_DEFAULT 0u
#define MTSV_DEV_SAMPLED_SA_ONLY 1u /* keep the file's row-sampled SA only (LF-walk locate) */
#define MTSV_DEV_NO_KMER_TABLE 2u   /* no seed-suffix interval table */
#define MTSV_DEV_PACK_ON_DEVICE 4u /* pack on the device, below; combines freely with the other two */
int mtsv_index_to_device(mtsv_index *ix, int hip_device, uint32_t flags);

/* ---- packing on the device (k_pack.hip) ----------------------------------------------------------------------------
 * By default the host re-packs the file's BWT into rank blocks and its text into codes, on its threads, before the first
 * byte is uploaded.  With MTSV_DEV_PACK_ON_DEVICE the file's raw bytes cross instead -- bwt (n bytes), the six Occ arrays of
 * A C G T N $, then the text (n bytes), as temporaries in HBM -- and kernels pack them: per tile of 64 rank blocks a count, a
 * scan of the tiles' counts, the blocks, a check of every Occ checkpoint of the file against the blocks just written, and
 * the text's codes.  What is resident afterwards is byte for byte what the host pack uploads -- rank blocks, text codes,
 * every scalar, device_bytes -- and so is everything built on top of it by the same kernels: the full suffix array, the
 * k-mer table, its width, its kept levels and tags.  Every temporary is freed before the table's width is decided from
 * the free HBM.  The SA samples, the bins and the bin lookup table are prepared on the host in both cases.
 * Errors are the host pack's, text and code: "format: bwt holds a symbol outside ACGTN$", "format: bwt holds no sentinel",
 * "format: Occ checkpoint J disagrees with the bwt" with J the smallest such checkpoint; nothing stays allocated then.
 * Environment, read at every upload: MTSV_DEV_PACK=device packs on the device without the flag (for an A/B of the command
 * line and the tools; the flag an index is resident with is the one that was passed); MTSV_PACK_TILE=1..64 (a power of
 * two) moves the tile edges, for tests. */

/* For tests, like mtsv_batch_download_reads: a look inside the index resident on `hip_device`.  *out is malloc'd
 * (mtsv_free) and holds *bytes bytes: the device's array as it is, or for MTSV_DEVPART_HEADER one mtsv_device_header.
 * MTSV_E_ARG when the index is not resident there or the part is unknown. */
#define MTSV_DEVPART_HEADER 0   /* mtsv_device_header, below */
#define MTSV_DEVPART_BLOCKS 1   /* n_blocks rank blocks of 64 bytes */
#define MTSV_DEVPART_TEXT 2     /* (n + 15) / 16 * 16 + 32 codes, 7 behind n */
#define MTSV_DEVPART_SA_SAMPLE 3
#define MTSV_DEVPART_BINS 4     /* n_bins x {start, end, tax_id, gi} u32 */
#define MTSV_DEVPART_BIN_END 5
#define MTSV_DEVPART_BIN_LUT 6
#define MTSV_DEVPART_TEXT_SECTORS 7 /* the text's whole array: (n + 63) / 64 * 64 + 64 codes, 7 behind n */
typedef struct {
    uint32_t n, n_blocks;
    uint32_t C[5];             /* less[] of A, C, G, T, N */
    uint32_t sentinel_row;
    uint32_t sa_s, sa_pow2_shift;
    uint32_t n_bins, bin_lut_shift;
    uint32_t kmer_k;           /* 0: no table */
    uint32_t sa_full;          /* 1 when the full suffix array is resident */
    uint32_t packed_on_device; /* 1 when this upload packed on the device (by the flag or by MTSV_DEV_PACK) */
    uint32_t _pad;
    uint64_t device_bytes;
    /* times of the upload in ms.  pack_ms: the host pack by the host's clock, or the pack kernels by device events;
     * copy_ms: the host-to-device copies by the host's clock around the synchronous calls; accel_build_ms: the full
     * suffix array and the k-mer table, by device events */
    float pack_ms, copy_ms, accel_build_ms;
    float _pad2;
} mtsv_device_header;
int mtsv_index_download_device(mtsv_index *ix, int hip_device, int part, void **out, uint64_t *bytes);

/* ---- the hot path ----------------------------------------------------------------------- */
/* bases: concatenated raw read bytes (any case, any byte), read_off[n_reads+1].
 * *hits is ordered by (read, strand, rank order of the reference's candidate loop) and owned by
 * the caller (mtsv_hits_free); the array is page-locked host memory from a pool the library
 * recycles (the hits of each slice are copied there while later slices still compute). */
int mtsv_bin_batch(mtsv_index *ix, int hip_device, const uint8_t *bases, const uint64_t *read_off,
                   uint64_t n_reads, const mtsv_params *params, mtsv_hit **hits, uint64_t *n_hits);
void mtsv_hits_free(mtsv_hit *hits);
/* Page-locked host memory for read buffers (the reference fills plain Vec<u8> buffers, src/binner.rs:21-66; a host
 * that keeps its parsed reads in memory from here spares every call a copy).  mtsv_bin_batch*, mtsv_batch_upload and
 * mtsv_batch_run_host recognise bases that lie in such memory and let the GPU's copy engine read them where they
 * are; any other memory is staged through the library's own page-locked buffers first (a host memcpy per slice).
 * mtsv_host_register page-locks memory the caller already owns (page-aligned ranges are best; it must be
 * unregistered before it is freed).  Both work without an index or a batch; NULL / an error code when no HIP
 * device is usable. */
void *mtsv_host_alloc(size_t bytes);
void mtsv_host_free(void *p);
int mtsv_host_register(void *p, size_t bytes);
int mtsv_host_unregister(void *p);
/* ---- several GPUs of one node (no collective: reads are independent) --------
 * Mode A -- the reference's single-index workflow (README.md:69-73) on several GPUs: the index is replicated
 * on every listed device, the reads are cut into n_devices contiguous blocks, one host thread and workspace per
 * entry, hits concatenated in read order (hit.read indexes the whole batch).  A device may be listed more than
 * once (two workspaces on it).  Output identical to mtsv_bin_batch. */
int mtsv_bin_batch_multi(mtsv_index *ix, const int *devices, int n_devices, const uint8_t *bases,
                         const uint64_t *read_off, uint64_t n_reads, const mtsv_params *params,
                         mtsv_hit **hits, uint64_t *n_hits);
/* Mode B -- the chunked-database workflow (mtsv-chunk, then one binner run per chunk, then mtsv-collapse:
 * README.md:189, src/collapse.rs:597-625): chunk k of the database is resident on devices[k], every chunk sees
 * every read, and the per-chunk hit lists are merged per read (chunk order within a read).
 * mtsv_format_results on the merged list writes the line mtsv-collapse would produce from the per-chunk
 * result files: smallest edit per (read, TaxId). */
int mtsv_bin_batch_chunks(mtsv_index *const *chunks, const int *devices, int n_chunks,
                          const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads,
                          const mtsv_params *params, mtsv_hit **hits, uint64_t *n_hits);
/* reads per device workspace mtsv_bin_batch creates (and keeps) for a host batch of n_reads reads; larger
 * batches stream through it in slices */
uint64_t mtsv_bin_batch_workspace_reads(uint64_t n_reads);

/* The same path with the batch resident in HBM (what bench.py times).  The index must already be
 * on `hip_device`.  max_hits_ws = seed-hit workspace entries (0 = default). */
int mtsv_batch_create(mtsv_index *ix, int hip_device, uint64_t max_reads, uint64_t max_bases,
                      uint64_t max_hits_ws, mtsv_batch **out);
/* The same with the number of LANES chosen: a host batch (mtsv_batch_run_host*) is worked off in ranges, `lanes` of them
 * at a time, each on a stream and a set of work arrays of its own (0: the default, three).  A host that keeps several
 * calls in flight on one device -- a workspace per worker thread, as mtsv-binner does -- asks for one lane each: its
 * calls are what overlap.  (No counterpart in the reference: src/binner.rs:57-76 is a pool of CPU threads.) */
int mtsv_batch_create_lanes(mtsv_index *ix, int hip_device, uint64_t max_reads, uint64_t max_bases,
                            uint64_t max_hits_ws, int lanes, mtsv_batch **out);
/* Make the workspace ready for host batches of up to n_reads reads / n_bases bases: what mtsv_batch_run_host* would
 * otherwise size on its first calls (device arenas, the page-locked offset table, a result array) is created now, and
 * with warm_read_len > 0 a small batch of reads of that length sampled from the index runs through every kernel (the
 * first launch of a kernel loads its code object).  Part of the device set-up, like mtsv_index_to_device. */
int mtsv_batch_reserve_host(mtsv_batch *b, uint64_t n_reads, uint64_t n_bases, uint32_t warm_read_len);
/* Order in which the two acceptance predicates of index.rs:406,410 are evaluated (results identical):
 *   MTSV_VERIFY_REFERENCE   SW prefilter score and edit distance for every verified candidate (default)
 *   MTSV_VERIFY_EDIT_FIRST  edit distance first; for reads <= 253 bases edits <= ED implies the SW
 *                           threshold, so the SW sweep is not needed (longer reads use REFERENCE)
 * The environment variable MTSV_VERIFY=reference|edit_first sets the default of new batches. */
#define MTSV_VERIFY_REFERENCE 0
#define MTSV_VERIFY_EDIT_FIRST 1
int mtsv_batch_set_verify_mode(mtsv_batch *b, int mode);
/* process-wide default of workspaces created from now on (also those mtsv_bin_batch* keep); the environment
 * variable, when set, wins */
int mtsv_set_default_verify_mode(int mode);
int mtsv_batch_upload(mtsv_batch *b, const uint8_t *bases, const uint64_t *read_off,
                      uint64_t n_reads);
int mtsv_batch_run(mtsv_batch *b, const mtsv_params *params); /* synchronous: returns when done */
/* upload + run in one call for host buffers of any size: the reads are cut into slices of at most
 * the workspace's max_reads / max_bases, and slice k+1 is copied to the device while slice k runs
 * (two input buffers, a copy stream), so the PCIe transfer hides behind the kernels.  Hit `read`
 * fields index the whole host batch.  Stats cover all slices. */
int mtsv_batch_run_host(mtsv_batch *b, const uint8_t *bases, const uint64_t *read_off,
                        uint64_t n_reads, const mtsv_params *params);
/* The same for a batch that lies in n_parts pieces (a host that parses its input in blocks hands several blocks to one
 * call -- larger passes on the device -- without putting them together first): part k holds n_reads[k] reads, bases[k]
 * with read_off[k][0 .. n_reads[k]]; the reads are numbered through the parts in order, and mtsv_batch_download returns
 * one hit list over all of them.  (The reference has no such call: its worker closure takes one read,
 * src/binner.rs:77-131.) */
int mtsv_batch_run_host_parts(mtsv_batch *b, int n_parts, const uint8_t *const *bases, const uint64_t *const *read_off,
                              const uint64_t *n_reads, const mtsv_params *params);
int mtsv_batch_stats_get(const mtsv_batch *b, mtsv_batch_stats *st);

/* ---- taxa report: per-TaxID read counts (mtsv-collapse --report, src/collapse.rs:43-62,120-146) ---------------
 * Per read with at least one hit (the hits mtsv_batch_download returns for it): summary = {tax_id -> smallest edit over
 * the read's hits, both strands}.  With m the smallest edit of the summary, every TaxID of it counts the read once:
 *   only_hit   the summary has one entry
 *   only_best  its edit is m and no other entry's is
 *   tied_best  its edit is m and another entry's is too
 *   not_best   its edit is above m
 * total_reads counts the reads with a hit.  The counts are summed on the device, pass by pass, from the hits while they
 * are in HBM (k_report.hip); they do not depend on how a batch was cut into passes, lanes or calls.  mtsv-collapse keys
 * reads by their text ID and so merges records that carry the same ID; here every read counts by itself. */
typedef struct {
    uint32_t tax_id;
    uint32_t _pad;
    uint64_t only_hit, only_best, tied_best, not_best;
} mtsv_taxon_stats;
/* on != 0: every run of this workspace from now on (mtsv_batch_run, _run_host, _run_host_parts) adds its reads to the
 * workspace's report.  Off by default, and off costs nothing: no allocation, no launch.  What the report needs on the
 * device (the index's distinct TaxIDs, four counters each) is created when it is first switched on; the environment
 * variable MTSV_REPORT_DENSE_MAX, read then, moves the number of taxa up to which the workgroups count in one LDS
 * counter per (TaxID, category) instead of an LDS hash table (tests; at most 4095); MTSV_REPORT_HASH_SLOTS shrinks that table (tests). */
/* Switching the report off keeps what it has counted: runs while it is off add nothing, and switching it on again goes on
 * from those counts (only reset != 0 of mtsv_batch_taxa_report zeroes them). */
int mtsv_batch_set_taxa_report(mtsv_batch *b, int on);
/* Rows for every TaxID with a non-zero counter, ascending tax_id; the caller frees *rows with mtsv_free.  device_ms
 * (may be NULL): device time of the report's kernels since the last reset.  reset != 0 zeroes the accumulation after
 * reading it.  MTSV_E_ARG when the report is not on. */
int mtsv_batch_taxa_report(mtsv_batch *b, mtsv_taxon_stats **rows, uint64_t *n_rows, uint64_t *total_reads,
                           float *device_ms, int reset);
/* Sum of two reports (several workspaces that shared one input): rows of the same TaxID add up.  Both inputs ascending
 * by tax_id; *out is malloc'd (mtsv_free) and ascending.  Host only. */
int mtsv_merge_taxa_reports(const mtsv_taxon_stats *a, uint64_t n_a, const mtsv_taxon_stats *b, uint64_t n_b,
                            mtsv_taxon_stats **out, uint64_t *n_out);
/* write_taxa_report (src/collapse.rs:716-750): the header line and one line per row, every count followed by its
 * percentage of max(total_reads, 1) with two decimals, then the row's sum and its percentage.  *out is malloc'd
 * (mtsv_free).  Host only, needs no device. */
int mtsv_format_taxa_report(const mtsv_taxon_stats *rows, uint64_t n_rows, uint64_t total_reads, char **out,
                            uint64_t *out_len);

/* ---- match flags: did a read get a hit (mtsv-partition, src/bin/mtsv-partition.rs:34-54) ------------------------
 * mtsv-partition splits a read file by whether a read's ID occurs in a results file: it parses the results text back
 * into a hash set of IDs (:34-54) and reads the FASTX input a second time.  The binner decides the same question on the
 * device: a read is MATCHED when the run returns at least one hit for it, on either strand, under the caller's
 * mtsv_params.  With the flags on, every committed pass of a run sets one bit per matched read in a bitmap over the
 * run's reads (k_match.hip), and counts them.  The flags describe ONE run -- the last mtsv_batch_run, _run_host or
 * _run_host_parts of the workspace; they do not add up over runs as the taxa report does.  Every read counts by itself
 * here; mtsv-partition keys reads by their text ID, so there two records that carry the same ID share a fate.
 *   MTSV_MATCH_OFF        the default: no allocation, no launch, nothing changes
 *   MTSV_MATCH_WITH_HITS  the hits as always, plus the flags
 *   MTSV_MATCH_ONLY       the flags only (read depletion): the passes skip the scan and gather of their hits, no result
 *                         array is kept or copied, mtsv_batch_download returns zero hits and n_hits of the stats is 0
 *                         (the other counters keep their meaning for the work that was done).  The selection loop stops
 *                         at a strand's first accepted candidate: whether there is one does not depend on
 *                         max_assignments (src/index.rs:384-428 pushes a hit before it looks at the limit).
 * MTSV_MATCH_ONLY and the taxa report (which reads gathered hits) exclude each other: whichever is asked for second
 * fails with MTSV_E_ARG. */
#define MTSV_MATCH_OFF 0
#define MTSV_MATCH_WITH_HITS 1
#define MTSV_MATCH_ONLY 2
int mtsv_batch_set_match_flags(mtsv_batch *b, int mode);
/* The flags of the last run: bit (r & 63) of (*words)[r >> 6] is read r in that call's numbering (through the parts of
 * mtsv_batch_run_host_parts in order); bits at and above *n_reads are 0; *words holds (*n_reads + 63) / 64 words (at
 * least one) and is malloc'd (mtsv_free); *n_matched is the number of set bits, counted on the device.  No run since the
 * flags were switched on: *n_reads is 0.  MTSV_E_ARG when the mode is MTSV_MATCH_OFF. */
/* "Switched on" is the step from MTSV_MATCH_OFF to either other mode, and for the assignments from MTSV_ASSIGN_OFF: a change
 * between the two modes that are on keeps what the last run left.
 * What the observers of a workspace's LAST RUN return -- mtsv_batch_download, _stats_get, _match_flags, _download_assignments*,
 * _format_text -- is defined from the moment a run (or a merge into the workspace) completes until the workspace is given
 * other reads (mtsv_batch_upload, _take_reads, _copy_reads, _take_unique as dst) or a run on it fails; in between it is not
 * defined, and callers look again after the next run.  A run that returns an error (MTSV_E_LIMIT for a read above 32767
 * bases, MTSV_E_ARG for bad parameters) leaves the resident batch and its read map as they were; the taxa report has taken
 * the passes that completed.  The hits of a host batch (mtsv_batch_run_host*) are handed out once: a second
 * mtsv_batch_download after the same call is not defined (the assignments may be downloaded again, below).  The hits that a
 * resident run (mtsv_batch_run) or a merge gathered stay in HBM until the next run, merge or change of the reads, and a change
 * of the flags' or the assignments' mode does not touch them: mtsv_batch_download copies them out again, as often as it is
 * called (zero hits while the mode is MTSV_ASSIGN_ONLY, and after a run in MTSV_MATCH_ONLY, which gathered none).  After a
 * host batch a change of mode leaves mtsv_batch_download undefined until the next run; the one case that is refused is named
 * at mtsv_batch_download_assignments. */
int mtsv_batch_match_flags(mtsv_batch *b, uint64_t **words, uint64_t *n_reads, uint64_t *n_matched);

/* ---- chaining workspaces: the unmatched (matched) reads of one run as the input of another, on the device ----------
 * Read depletion followed by binning -- a filter index (a host genome), then the database -- goes through a file in the
 * reference's workflow: mtsv-partition writes the unmatched reads (src/bin/mtsv-partition.rs:56-93), a second
 * mtsv-binner run parses them again.  Here both indexes are resident on one device, a workspace each, and
 * mtsv_batch_take_reads hands the reads over in HBM (k_compact.hip): dst's resident batch becomes the reads of src's
 * last run whose match flag is clear (MTSV_KEEP_UNMATCHED) or set (MTSV_KEEP_MATCHED), in order, as if they had been
 * given to mtsv_batch_upload -- no base crosses PCIe again, no flag goes to the host; the host reads 24 bytes of counts
 * and four bytes per survivor (their offsets).  dst also receives a READ MAP, survivor -> read number in src's run, and
 * mtsv_batch_run on dst writes the mapped number into the `read` field of every hit, so the hits are numbered like
 * the caller's batch and stay ordered by it.  dst's own match flags and taxa report stay per resident read
 * (mtsv_batch_read_map translates).  A workspace filled this way can be a source in turn, and the maps compose: the
 * reads no chunk of a filter matches are a chain of MTSV_KEEP_UNMATCHED steps, each on fewer reads.
 * src: match flags on, in either mode, and a completed run whose reads are still in HBM -- mtsv_batch_upload +
 * mtsv_batch_run, or a host batch of mtsv_batch_run_host* that fitted one input segment (3 GiB of bases; a larger one
 * took turns through two segments and has lost its first reads: MTSV_E_ARG).  Also MTSV_E_ARG: flags off, no such run,
 * dst == src, workspaces of different devices, a bad `keep`, more survivors (or bases) than dst was created for -- dst
 * is then as it was.  Synchronous.  device_ms (may be NULL): device time of the kernels.  mtsv_batch_upload and
 * mtsv_batch_run_host* on dst drop the map.  (Both indexes share the device's HBM: mtsv_index_to_device of the second
 * may settle for a narrower k-mer table, or fail for want of memory.) */
#define MTSV_KEEP_UNMATCHED 0
#define MTSV_KEEP_MATCHED 1
int mtsv_batch_take_reads(mtsv_batch *dst, mtsv_batch *src, int keep, uint64_t *n_kept, uint64_t *bases_kept,
                          float *device_ms);
/* ---- chunked databases on one device: the same reads in several workspaces, their runs merged in HBM -----------------
 * A database cut with mtsv-chunk is binned chunk by chunk and a read's hits come from several chunks; what is counted per
 * read -- the taxa report, the match flags -- has to see them together (a TaxID's smallest edit may come from any chunk,
 * and a read matched in two chunks is one matched read).  With every chunk resident on one device, a workspace each:
 * the reads go up once (mtsv_batch_upload, or mtsv_batch_take_reads behind a filter), mtsv_batch_copy_reads gives them
 * to the other chunks' workspaces, every workspace runs (mtsv_batch_run), and mtsv_batch_merge_runs puts the hits
 * together per read in a further workspace, the collector (k_merge.hip).  K chunks take K + 1 workspaces of HBM.
 *
 * mtsv_batch_copy_reads: dst's resident batch becomes a copy of src's -- codes (or the bases as uploaded), offsets,
 * longest read, read map -- as if the same reads had been handed to dst: mtsv_batch_run on it skips the normalisation
 * when src held codes and writes mapped read numbers when src was mapped.  src holds a resident batch from
 * mtsv_batch_upload, _take_reads, _copy_reads, or a host batch that fitted one input segment; it needs no match flags and
 * no completed run.  Everything moves from HBM to HBM; the host copies its own offset table.  MTSV_E_ARG, with dst as it
 * was: dst == src, different devices, nothing resident in src, more reads or bases than dst was created for.
 * device_ms (may be NULL): device time of the copies. */
int mtsv_batch_copy_reads(mtsv_batch *dst, mtsv_batch *src, float *device_ms);
/* mtsv_batch_merge_runs: the last runs of srcs[0 .. n_srcs), which all hold the same reads, merged per read into dst.
 * Afterwards mtsv_batch_download(dst) returns, per read in read order, the hits of srcs[0], then of srcs[1], and so on,
 * every source in its own order: the list mtsv_bin_batch_chunks returns.  mtsv_batch_stats_get(dst) gives n_reads and
 * n_hits of the merge, the rest 0.  With dst's match flags on (MTSV_MATCH_WITH_HITS) they describe the merge: bit j is
 * set when resident read j has a hit in any source, and n_matched is counted on the device.  With dst's taxa report on,
 * the merged reads are added to it once; the report's TaxID list becomes the union of dst's index and every source's
 * (when a merge brings new TaxIDs the list and the counters so far are rebuilt, host work, and the dense / hashed tier is
 * decided again for the new size).  Sources are meant to run with their own reports off: those would count per chunk.
 * Sources: 1..64 workspaces of dst's device, each with a completed mtsv_batch_run on a resident batch whose hits are still
 * in HBM (a host batch is refused), none in MTSV_MATCH_ONLY (that mode gathers no hits); equal n_reads and equal offset
 * tables (the host copies are compared); all mapped or none (equal maps are the caller's business, mtsv_batch_copy_reads
 * gives them; the hits then carry the caller's numbers, flags and report stay per resident read).  They are only read and
 * keep their own results.  dst: any workspace of the device that is not among the sources and is not in
 * MTSV_MATCH_ONLY; its resident reads, if any, are not touched.  mtsv_batch_take_reads from a merged dst is refused
 * (MTSV_E_ARG): its flags describe reads it does not hold.  2^32 merged hits or more: MTSV_E_LIMIT (the scan's and the
 * report's offsets are 32 bits, as in a pass).  Every refusal leaves dst as it was: its last result, its counters, its
 * flags.  Only a refusal for want of device memory, with the report on, may come after the report's TaxID list has taken
 * the sources' TaxIDs; the counts so far are kept, the new rows are 0.  The host receives 16 bytes of counts; the hits
 * cross on mtsv_batch_download.  What the merge needs on the device is created by dst's first merge.
 * device_ms (may be NULL): device time of the merge kernels (bounds, sum, scan, copy). */
int mtsv_batch_merge_runs(mtsv_batch *dst, mtsv_batch *const *srcs, int n_srcs, float *device_ms);
/* (*map)[j] = the caller's number of resident read j (the identity after mtsv_batch_upload); malloc'd, mtsv_free */
int mtsv_batch_read_map(mtsv_batch *b, uint64_t **map, uint64_t *n_reads);
/* For tests, like mtsv_pack_bases: the resident batch as the kernels see it -- byte codes 0..4 (src/binner.rs:88-100)
 * and *n_reads + 1 offsets from 0; both malloc'd, mtsv_free.  MTSV_E_ARG when the workspace's last input was a host batch. */
int mtsv_batch_download_reads(mtsv_batch *b, uint8_t **codes, uint64_t **read_off, uint64_t *n_reads);
int mtsv_batch_download(mtsv_batch *b, mtsv_hit **hits, uint64_t *n_hits);

/* ---- assignments: one (TaxID, smallest edit) per read and TaxID (write_assignments, src/binner.rs:355-378) ----------
 * The default results line of mtsv-binner is READ_ID:TAXID=EDIT,...: the smallest edit per TaxID of the read, over both
 * strands, ascending by TaxID; mtsv-collapse --mode taxid builds the same across result files (src/collapse.rs:269-297).
 * With the assignments on, every committed pass reduces its gathered hits to that on the device (k_collapse.hip): one
 * 16-byte record per read and distinct TaxID.  Records are ordered like the hits -- by `read`, the caller's numbering,
 * ascending -- and inside a read by tax_id ascending as unsigned.  `read` is copied from the hit: on a workspace filled by
 * mtsv_batch_take_reads it is the caller's number.  In a collector (mtsv_batch_merge_runs into a workspace with the
 * assignments on) the reduction runs over the merged hits, all chunks together: what mtsv-collapse would write from the
 * per-chunk result files.  Assignments describe ONE run -- the last mtsv_batch_run, _run_host, _run_host_parts or
 * mtsv_batch_merge_runs into the workspace -- like the match flags and unlike the taxa report; a refused merge leaves
 * them as they were.
 *   MTSV_ASSIGN_OFF        the default: no allocation, no launch, nothing changes
 *   MTSV_ASSIGN_WITH_HITS  the hits as always, plus the assignments
 *   MTSV_ASSIGN_ONLY       the hits are gathered on the device (the collapse reads them, and so do the taxa report and
 *                          the match flags) but never copied to the host: mtsv_batch_download returns zero hits; the
 *                          stats keep their meaning, n_hits included
 * Grains (mtsv_batch_set_assignment_grain): the above is MTSV_GRAIN_TAXID.  MTSV_GRAIN_LONG keeps one 24-byte record per
 * distinct (tax_id, gi, offset) of the read with the triple's smallest edit, ascending by the triple -- the line of
 * --output-format long, READ_ID:TAXID-GI-OFFSET=EDIT,... (src/binner.rs:320-352); MTSV_GRAIN_TAXID_GI one per distinct
 * (tax_id, gi) with the lexicographically smallest (edit, offset) of the pair, ascending by the pair -- what mtsv-collapse
 * --mode taxid-gi makes of long files (src/collapse.rs:603-625), and in a collector over all chunks.  All fields compare as
 * unsigned.  Everything said of the 16-byte records holds for these.
 * Limits: one run's worth; offsets below 2^32 (no device index reaches them); not together with
 * MTSV_MATCH_ONLY, which gathers no hits -- whichever of the two is asked for second fails with MTSV_E_ARG; a bad mode is
 * MTSV_E_ARG; mtsv_bin_batch, _multi and _chunks do not produce assignments.  The taxa report and MTSV_MATCH_WITH_HITS
 * work beside every mode.  MTSV_COLLAPSE_LANE_MAX (1..16), MTSV_COLLAPSE_WAVE_MAX (..64) and MTSV_COLLAPSE_LDS_MAX (a power
 * of two, 2..4096; 2..2048 in the two wide grains, whose keys are 16 bytes) move the kernel's tier edges (tests); they are
 * read when the assignments are switched on. */
typedef struct {
    uint64_t read;
    uint32_t tax_id;
    uint32_t edit;
} mtsv_assignment; /* 16 bytes */
#define MTSV_ASSIGN_OFF 0
#define MTSV_ASSIGN_WITH_HITS 1
#define MTSV_ASSIGN_ONLY 2
int mtsv_batch_set_assignments(mtsv_batch *b, int mode);
/* The assignments of the last run.  *a is page-locked memory from the library's pool of result arrays, also when *n is 0;
 * the caller returns it with mtsv_free (which hands pool arrays back to the pool and frees everything else).  On
 * mtsv_batch_run_host* a finished range's records leave for that array on the result copy stream, in read order, while
 * later ranges still compute, as its hits do; this call then only hands the array out.  After a resident run or a merge,
 * and on a second call after the same run, the records are copied here from HBM stretch by stretch.  device_ms (may be
 * NULL): device time of the run's collapse kernels.  No run since the assignments were switched on: *n is 0.
 * MTSV_E_ARG when the mode is MTSV_ASSIGN_OFF.
 * A host batch run in MTSV_ASSIGN_ONLY keeps none of its hits: mtsv_batch_download after leaving that mode, without a new
 * run, is MTSV_E_ARG. */
int mtsv_batch_download_assignments(mtsv_batch *b, mtsv_assignment **a, uint64_t *n, float *device_ms);
/* The grain of the assignments.  Legal only while they are MTSV_ASSIGN_OFF (MTSV_E_ARG otherwise, and nothing changes): the
 * record arrays of a workspace hold one record size while they are on; switching off, changing the grain and switching on
 * again is allowed.  A bad grain is MTSV_E_ARG.  mtsv_batch_download_assignments is MTSV_E_ARG unless the grain is
 * MTSV_GRAIN_TAXID; mtsv_batch_download_assignments_gi is MTSV_E_ARG when it is, and when the mode is off; in everything else
 * (the pool array, also for *n == 0; mtsv_free; device_ms; a second call) the two calls are alike. */
#define MTSV_GRAIN_TAXID 0
#define MTSV_GRAIN_TAXID_GI 1
#define MTSV_GRAIN_LONG 2
int mtsv_batch_set_assignment_grain(mtsv_batch *b, int grain);
typedef struct {
    uint64_t read;
    uint32_t tax_id, gi, offset, edit;
} mtsv_assignment_gi; /* 24 bytes */
int mtsv_batch_download_assignments_gi(mtsv_batch *b, mtsv_assignment_gi **a, uint64_t *n, float *device_ms);
void mtsv_batch_free(mtsv_batch *b);

/* ---- folding runs: a chunked database larger than HBM, one chunk resident at a time -----------------------------------
 * mtsv_batch_merge_runs needs every chunk of a database resident at once, a workspace each and one more.  A database that
 * mtsv-chunk cut because it does not fit goes chunk by chunk instead: make chunk c resident, run the reads against it with
 * the assignments on, fold the run's assignment records into an mtsv_fold, free the workspace and the index, load chunk
 * c + 1.  The fold holds RECORDS, not hits: the sorted union of every list folded so far with one record per key -- what
 * mtsv-collapse makes of the per-chunk result files (src/collapse.rs:269-297, :603-625) -- so it is bounded by what the
 * final results file holds, at 16 or 24 bytes a record, and not by the sum of the chunks' hits.
 *   grain                key                           kept for a key that two lists hold
 *   MTSV_GRAIN_TAXID     (read, tax_id)                the smaller edit
 *   MTSV_GRAIN_LONG      (read, tax_id, gi, offset)    the smaller edit
 *   MTSV_GRAIN_TAXID_GI  (read, tax_id, gi)            the lexicographically smaller (edit, offset)
 * All fields compare as unsigned.  The merge is global (k_fold.hip: a merge path over both lists), not per read: it does not
 * depend on the reads' numbering or count, and a read with thousands of records costs what thousands of reads with one do.
 * The order in which lists are folded does not change the result.  Everything counted per read is derived from the
 * accumulated records when asked for: the match flags (a read is matched when it has a record) and the taxa report
 * ({tax_id -> smallest edit} per read, the categories of mtsv_taxon_stats).
 * A fold is bound to a device and a grain, not to an index, and keeps no pointer to a workspace: after mtsv_fold_add_run
 * returns, src and its index may be freed.  The accumulator lies in two arrays that take turns and grow together, by
 * reallocation, when a fold needs more room; 2^32 records or more before equal keys are joined is MTSV_E_LIMIT (the scan's
 * offsets are 32 bits, as in a pass).  Every refusal leaves the fold as it was.  MTSV_FOLD_TILE (a power of two, 2..1024),
 * read by mtsv_fold_create, moves the merge's tile size (tests).  With no fold created nothing is allocated or launched.
 *
 * mtsv_fold_create: MTSV_E_ARG for a bad grain, MTSV_E_DEVICE when hip_device is no usable device.
 * mtsv_fold_reset: the fold is empty, its reads are numbered below n_reads (the caller's numbering: the flags have n_reads
 *   bits), its TaxID union is empty.  A new fold is as after mtsv_fold_reset(f, 0).
 * mtsv_fold_add_run: folds the assignments of src's last run.  src: a workspace of the fold's device whose assignments are
 *   on, in either mode, at the fold's grain, and whose last run was mtsv_batch_run on a resident batch or
 *   mtsv_batch_merge_runs (a host batch of mtsv_batch_run_host* is refused: its records left for the host range by range);
 *   anything else is MTSV_E_ARG.  The records, which may lie in several stretches of the workspace's lanes, are put next to
 *   each other in HBM first.  On a workspace filled by mtsv_batch_take_reads / _copy_reads they carry the caller's numbers,
 *   which is all a chain needs.  The TaxIDs of src's index join the fold's union, the list the report's rows come from; a
 *   merged collector's records come from every chunk of its merge, so there the TaxIDs are read from the records (they
 *   cross to the host once).
 * mtsv_fold_add_records: uploads and folds n host records of the fold's grain (mtsv_assignment, or mtsv_assignment_gi in
 *   the two wide grains) -- from an earlier run, another device, a file parsed elsewhere.  Checked on the host: keys
 *   strictly ascending and read < n_reads, MTSV_E_ARG otherwise.  Their TaxIDs join the union.
 * device_ms (may be NULL): device time of the fold's kernels (count, scan, write).
 * mtsv_fold_download / _download_gi: the accumulated records in key order.  *a is page-locked memory from the library's pool
 *   of result arrays, also when *n is 0; the caller returns it with mtsv_free.  mtsv_fold_download on a wide grain and
 *   mtsv_fold_download_gi on MTSV_GRAIN_TAXID are MTSV_E_ARG.  mtsv_format_assignments* write the result lines.
 * mtsv_fold_taxa_report: rows as mtsv_batch_taxa_report gives them (non-zero rows, ascending tax_id, mtsv_free), equal to
 *   those of a collector that merged the same runs; *total_reads: the reads with a record.  Reports of several folds over
 *   disjoint reads add up with mtsv_merge_taxa_reports.  A record whose TaxID is not in the union is counted on the device
 *   and makes the call fail, MTSV_E_DEVICE (an internal error: every way in adds its TaxIDs).
 * mtsv_fold_match_flags: as mtsv_batch_match_flags, over the n_reads of the reset; *n_matched is counted on the device.  A
 *   record whose read is at or above n_reads (only mtsv_fold_add_run can bring one) makes the call fail, MTSV_E_DEVICE. */
typedef struct mtsv_fold mtsv_fold;
int mtsv_fold_create(int hip_device, int grain, mtsv_fold **out);
void mtsv_fold_free(mtsv_fold *f);
int mtsv_fold_reset(mtsv_fold *f, uint64_t n_reads);
int mtsv_fold_add_run(mtsv_fold *f, mtsv_batch *src, float *device_ms);
int mtsv_fold_add_records(mtsv_fold *f, const void *records, uint64_t n, float *device_ms);
int mtsv_fold_count(const mtsv_fold *f, uint64_t *n);
int mtsv_fold_download(mtsv_fold *f, mtsv_assignment **a, uint64_t *n);
int mtsv_fold_download_gi(mtsv_fold *f, mtsv_assignment_gi **a, uint64_t *n);
int mtsv_fold_taxa_report(mtsv_fold *f, mtsv_taxon_stats **rows, uint64_t *n_rows, uint64_t *total_reads, float *device_ms);
int mtsv_fold_match_flags(mtsv_fold *f, uint64_t **words, uint64_t *n_reads, uint64_t *n_matched);

/* ---- result text folded on the device: per-chunk result files that already exist ------------------------------------------
 * The documented way to run a chunked database is one mtsv-binner job per chunk, often on other nodes or days, and
 * mtsv-collapse over the per-chunk result files.  mtsv_fold_add_run needs the run in this process; this call takes the
 * run's TEXT: it is the inverse of mtsv_fold_format_text, and what mtsv-collapse --on-gpu is built on.
 *   hits                 the hit parts of n_lines result lines laid end to end -- what stands behind the last ':' of a line,
 *                        without ID, ':' or line end
 *   line_off[n_lines+1]  ascending from 0: line j is hits[line_off[j] .. line_off[j + 1]), TOKEN(,TOKEN)* or nothing
 *   line_read[n_lines]   the number the caller gave the line's read ID, strictly ascending over the non-empty lines and
 *                        below the n_reads of the last mtsv_fold_reset (a file that names an ID on several lines, or whose
 *                        lines are not in the order of the numbering, is the caller's to cut and reorder)
 * A token is T=E, T-G=E or T-G-O=E, every number 1 to 10 decimal digits with value <= 4294967295, as the binners and
 * mtsv-collapse write them.  A fold of MTSV_GRAIN_TAXID takes all three shapes and uses T and E; the two wide grains need
 * T-G-O=E.  Inside a line the tokens ascend by the key of the fold's grain (equal keys may follow each other) -- long-format
 * lines are ordered by (tax, gi, offset), so they do, at every grain.  A run of adjacent tokens with one key becomes one
 * record with the smallest edit, at MTSV_GRAIN_TAXID_GI the smallest (edit, offset): the list is what k_collapse leaves of a
 * run, and it goes the way mtsv_fold_add_run's list goes.  No record crosses to the host or comes from it.
 * The kernels (k_parse.hip) are byte-parallel, then record-parallel: a workgroup owns a tile of bytes, a byte starts a token
 * when it begins a non-empty line or follows a ',', every token is parsed by the lane of its first byte, the runs of equal
 * keys are found by comparing neighbours, scanned, and reduced with one 64-bit atomic minimum per token.  A line of
 * thousands of tokens costs what thousands of short lines do.  MTSV_PARSE_TILE (a power of two, 64..16384 bytes), read by
 * mtsv_fold_create, moves the tile size (tests).  The arrays of the call grow by reallocation and are kept by the fold.
 * *n_tokens, *n_records (may be NULL): the tokens of the call and the records they made.  device_ms (may be NULL): device
 * time of the parse kernels and of the fold's.  The records' TaxIDs join the union (they cross to the host, 4 bytes each).
 * Refusals, all before the accumulator is touched -- the fold is as it was, mtsv_last_error names the first such line:
 *   MTSV_E_FORMAT  a token outside the grammar above (a trailing or doubled ',' makes an empty one), or, in a wide grain,
 *                  without GI and offset; offsets of 2^32 and above are outside it
 *   MTSV_E_ARG     a line whose keys descend; a line_read not above the previous non-empty line's, or at or above n_reads;
 *                  line_off that does not start at 0 or descends; a null array
 *   MTSV_E_LIMIT   2^32 tokens or more in one call; a fold that would hold 2^32 records or more
 * n_lines == 0 and empty lines fold nothing.  Not done here: mtsv-binner --fold-on-gpu starting from an earlier results file,
 * which this call makes possible. */
int mtsv_fold_add_text(mtsv_fold *f, const char *hits, const uint64_t *line_off, const uint32_t *line_read, uint64_t n_lines,
                       uint64_t *n_tokens, uint64_t *n_records, float *device_ms);

/* ---- result lines written on the device: the results file from records that never leave HBM as records ------------------
 * mtsv_format_assignments* walk downloaded records on a host thread.  These two calls write the same bytes on the device
 * (k_text.hip) from records that lie in HBM already, and what crosses to the host is the text: one line per read that has a
 * record, READ_ID:TAXID=EDIT,... from MTSV_GRAIN_TAXID records and READ_ID:TAXID-GI-OFFSET=EDIT,... from the two wide grains,
 * byte for byte what mtsv_format_assignments / mtsv_format_assignments_gi make of the same records and IDs.  ids and id_off
 * are what those take: the NUL-separated read IDs and id_off[n_reads + 1]; an ID is strnlen within its slot, which may be
 * NUL-padded or filled to its last byte with no NUL.
 * The kernels are record-parallel, not read-parallel: a record's bytes are its read's ID and ':' when it is the first of
 * its read, its fields, and ',' or '\n'; their lengths are measured (digit counts by comparison), scanned to 64-bit offsets,
 * and a workgroup writes the text of its tile of records through LDS.  A read with thousands of records costs what
 * thousands of reads with one record do.  MTSV_TEXT_TILE (a power of two, 2..1024) moves the tile size (tests); it is read
 * by mtsv_fold_create, and by a workspace's first mtsv_batch_format_text.  With neither call made nothing is allocated or
 * launched.
 *
 * mtsv_fold_format_text: the accumulated records of the fold, in its grain.  n_reads must be the n_reads of the last
 *   mtsv_fold_reset, MTSV_E_ARG otherwise.  The fold is not changed: its records, report and flags are as before.
 * mtsv_batch_format_text: the assignments of the workspace's last run, in its grain.  The assignments must be on, in either
 *   mode, and the last run mtsv_batch_run on a resident batch or mtsv_batch_merge_runs -- the sources mtsv_fold_add_run
 *   accepts; records that lie in several stretches of the workspace's lanes are put next to each other in HBM first.  A host
 *   batch of mtsv_batch_run_host* is MTSV_E_ARG (its records left for the host range by range), and so are assignments
 *   that are off and a workspace with no run yet.  On a workspace filled by mtsv_batch_take_reads / _copy_reads the records
 *   carry the caller's numbers: ids and n_reads are then the caller's.
 * Both: *text is page-locked memory from the library's pool of result arrays, also when *len is 0; it holds *len + 1 bytes
 *   with a NUL at *len, and the caller returns it with mtsv_free.  device_ms (may be NULL): device time of the kernels
 *   (measure, scan, write).  A null ids, id_off, text or len is MTSV_E_ARG.  Counted on the device, and MTSV_E_ARG with
 *   nothing returned: a record whose read is at or above n_reads; an ID slot that does not lie inside the ID bytes (id_off
 *   must ascend, id_off[n_reads] is the length of ids) or is longer than 2^20 bytes.  Every refusal leaves the fold or the
 *   workspace as it was.  The order of the records is not checked: every source keeps its records in key order.
 * Limits: one call's worth -- the IDs of all n_reads reads go up with every call, also of reads that have no record, and the
 *   text of a call lies in HBM before it is copied; fewer than 2^32 records.
 * Out of scope: text per range of a host batch (mtsv_batch_run_host*).  It needs the IDs on the device before the ranges
 *   finish and touches the lanes' staging; such a run's lines come from mtsv_format_assignments*. */
int mtsv_fold_format_text(mtsv_fold *f, const char *ids, const uint64_t *id_off, uint64_t n_reads, char **text, uint64_t *len,
                          float *device_ms);
int mtsv_batch_format_text(mtsv_batch *b, const char *ids, const uint64_t *id_off, uint64_t n_reads, char **text, uint64_t *len,
                           float *device_ms);

/* ---- identical reads binned once (dedup.hip, k_dedup.hip) ----------------------------------------------------------------
 * The result of binning is a function of a read's normalised codes and the parameters, so a batch that holds a sequence many
 * times (PCR and optical duplicates, rRNA, amplicons) needs the search once per distinct sequence.  Two reads are IDENTICAL
 * when their lengths are equal and every code (0..4 after normalisation: `acgt` equals `ACGT`, `R` equals `N`) is equal; no
 * reverse complement, no prefix relation.  For every resident read j, rep(j) is the smallest resident index whose read is
 * identical to j: exact and deterministic, whatever the hash function does.
 * An mtsv_dupmap is bound to a device and holds what the last mtsv_batch_take_unique found.  MTSV_DEDUP_HASH_BITS (0..64,
 * default 64: only that many low bits of the hash are used, for the start slot and the tag alike; 0 puts every read on one
 * probe chain) and MTSV_FAN_TILE (a power of two, 64..1024: the output records a workgroup of the expansion owns) are read by
 * mtsv_dupmap_create (tests); results do not depend on either.  With no map created nothing is allocated or launched.
 *
 * mtsv_dupmap_create: MTSV_E_DEVICE when hip_device is no usable device.
 * mtsv_batch_take_unique: dst's resident batch becomes the representatives (the reads with rep(j) == j) of src's resident batch,
 *   in order, as if they had been uploaded, held as codes; its read map (survivor -> the caller's number) is composed with
 *   src's when src is mapped, exactly as mtsv_batch_take_reads does.  src needs a resident batch under the conditions of
 *   mtsv_batch_copy_reads; no run and no match flags.  m then holds, per resident read j of src, read[j], the caller's number
 *   of j (strictly ascending; the identity when src is unmapped), and rep[j], the caller's number of rep(j).  MTSV_E_ARG, with
 *   dst and m as they were: dst == src; different devices, or m of another device; nothing resident in src; more
 *   representatives or bases than dst was created for; NULL handles.  The host receives five counters and the survivors'
 *   offsets, no codes and no flags.  device_ms (may be NULL): hash, insert, resolve, scan and copy.  More than 2^30 reads is
 *   MTSV_E_LIMIT.  With MTSV_TRACE set when the map was created: one stderr line, `[dedup] ...`.
 * mtsv_dupmap_download: both arrays, malloc'd (mtsv_free), *n_reads entries each; *n_reads is 0 before any take.
 * mtsv_fold_expand: dst becomes a fold as after mtsv_fold_reset(dst, n_reads of src) that holds, for every entry j of m, the
 *   records src holds for read rep[j] with `read` replaced by read[j] (key order holds because read[] ascends); its TaxID union
 *   is src's.  All three grains; src is not changed.  Everything a fold offers then works on dst.  Every record of src must
 *   belong to a read that is a representative in m: the records found for self-representing entries are counted, and a count
 *   that differs from src's is MTSV_E_ARG before anything is written.  Also MTSV_E_ARG, with dst as it was: dst == src,
 *   different grains or devices, an m that holds no take.  2^32 expanded records or more: MTSV_E_LIMIT.  device_ms (may be
 *   NULL): count, scan and write. */
/* A map whose last take was of a batch of zero reads holds a take of no entries: an empty src expands to an empty dst, any
 * other src is MTSV_E_ARG (its records belong to no representative). */
typedef struct mtsv_dupmap mtsv_dupmap;
int mtsv_dupmap_create(int hip_device, mtsv_dupmap **out);
void mtsv_dupmap_free(mtsv_dupmap *m);
int mtsv_batch_take_unique(mtsv_batch *dst, mtsv_batch *src, mtsv_dupmap *m, uint64_t *n_unique, uint64_t *bases_kept,
                           float *device_ms);
int mtsv_dupmap_download(const mtsv_dupmap *m, uint64_t **read, uint64_t **rep, uint64_t *n_reads, uint64_t *n_unique);
int mtsv_fold_expand(mtsv_fold *dst, mtsv_fold *src, const mtsv_dupmap *m, float *device_ms);

/* ---- taxonomy: per-read LCA and reads per clade ----------------------------------------------------------------------------
 * A fold answers "which TaxIDs did this read touch"; with a taxonomy it answers "which taxon IS this read, and how many reads
 * per species, genus or family".
 *
 * mtsv_taxonomy (host only, needs no device): an NCBI nodes.dmp.  Every line is split at '|', blanks and tabs around a field
 * are dropped, the first three fields are TaxID, parent TaxID and rank; further fields and a trailing '|' are ignored, so
 * `1 | 1 | no rank` loads like NCBI's `1\t|\t1\t|\tno rank\t|\t...\t|`.  Empty lines are skipped.  A node whose parent is
 * itself is a root; a parent that has no line of its own becomes an implied root of unknown rank; every root hangs under a
 * super-root with TaxID 0, so the LCA is total: taxa of different trees meet in 0.  Rank codes are the place of the rank
 * string among the file's distinct rank strings ascending by bytes; MTSV_RANK_UNKNOWN (printed "-") is the rank of the
 * super-root, of implied roots and of TaxIDs the file does not know.
 * mtsv_taxonomy_load: MTSV_E_IO for a file that cannot be read; MTSV_E_FORMAT, with mtsv_last_error naming the line or the
 *   TaxID, for a line of fewer than three fields, an ID that is not 1 to 10 digits or is above 4294967295, TaxID 0 (in either
 *   field), a TaxID listed twice, a cycle other than a self-parent.
 * mtsv_taxonomy_parent: the parent's TaxID -- 0 for roots, implied roots and the super-root itself -- and the rank code.  A
 *   TaxID the file does not know is a child of the super-root, as mtsv_fold_lca treats it: *parent 0, *rank
 *   MTSV_RANK_UNKNOWN.
 * mtsv_taxonomy_rank_name: the rank string of a code, "-" for MTSV_RANK_UNKNOWN and codes the file does not have; it lives
 *   as long as tx.
 *
 * mtsv_fold_lca: per read that has a record in f, with m the read's smallest edit, the TaxIDs of the records with
 * edit <= m + edit_slack (the sum saturates: 0 is the best taxa, 0xffffffff all taxa) ENTER, and the read's LCA is the deepest
 * node that is an ancestor-or-self of every entered TaxID.  A TaxID of f's union that tx does not know is a child of the
 * super-root: alone it is its own LCA, with anything else the LCA is 0.  All three grains; f is not changed.
 *   out (may be NULL): another fold of the same device at MTSV_GRAIN_TAXID.  It becomes a fold as after
 *     mtsv_fold_reset(out, n_reads of f) that holds exactly one record (read, LCA TaxID, m) per read with a record, its union
 *     the LCA TaxIDs present.  Everything a fold offers works on it: mtsv_fold_download, mtsv_fold_format_text (lines
 *     READ_ID:LCA=EDIT, a results file every tool reads), mtsv_fold_taxa_report (every row only_hit), mtsv_fold_match_flags
 *     (equal to f's).
 *   rows (may be NULL; needs n_rows and total_reads): one row per node with clade > 0, in preorder of the taxonomy -- a parent
 *     before its children, children ascending by TaxID as unsigned, the super-root first.  direct: the reads whose LCA is the
 *     node; clade: the sum of direct over its subtree; depth 0 for the super-root, 1 for roots.  *total_reads: the reads with
 *     a record, the super-root's clade.  malloc'd, mtsv_free.  The abundance at a rank is the rows of that rank.
 *   device_ms (may be NULL): device time of the kernels.
 * On the device (k_lca.hip): the host builds, per call and only when f's union or the taxonomy changed, the part of the
 * taxonomy the union needs -- the super-root, the union's TaxIDs, their ancestors -- numbered in preorder with the last node
 * of every subtree; then the LCA of a set is a walk up from its smallest member until the interval holds its largest, and a
 * clade is the difference of two prefix sums.  Five steps: heads, segmented minimum of edit, segmented min and max of the
 * entered node numbers, the walk, scan and clade.  MTSV_LCA_TILE (a power of two, 64..1024), read by mtsv_fold_create, moves
 * the tile size (tests); MTSV_LCA_TIMING=1 prints the steps' times to stderr.
 * MTSV_E_ARG, with both folds as they were: out == f, out on another device, out of a wide grain, a null f or tx, rows
 * without n_rows or total_reads.  An empty f gives an empty out and zero rows.  A record whose TaxID is not in f's union, or a
 * walk that does not end within the tree's depth, is an internal error, MTSV_E_DEVICE.
 * Not done here: mtsv-binner --fold-on-gpu, whose super-batches would need clade rows added across pieces.
 * mtsv_format_clade_report (host only): the TSV `taxid parent rank depth direct direct_pct clade clade_pct`, the rank as its
 * name; percentages of max(total_reads, 1) with two decimals, as mtsv_format_taxa_report computes its own.  tx may be NULL:
 * every rank is printed "-" then.  *out malloc'd, mtsv_free. */
#define MTSV_RANK_UNKNOWN 0xffffffffu
typedef struct mtsv_taxonomy mtsv_taxonomy;
typedef struct {
    uint64_t n_nodes;         /* lines of the file */
    uint64_t n_implied_roots; /* parents without a line */
    uint32_t n_ranks;         /* distinct rank strings */
    uint32_t max_depth;       /* the super-root is at 0, roots at 1 */
} mtsv_taxonomy_info_t;
int mtsv_taxonomy_load(const char *nodes_dmp, mtsv_taxonomy **out);
void mtsv_taxonomy_free(mtsv_taxonomy *tx);
int mtsv_taxonomy_info(const mtsv_taxonomy *tx, mtsv_taxonomy_info_t *info);
int mtsv_taxonomy_parent(const mtsv_taxonomy *tx, uint32_t tax_id, uint32_t *parent, uint32_t *rank);
const char *mtsv_taxonomy_rank_name(const mtsv_taxonomy *tx, uint32_t rank);
typedef struct {
    uint32_t tax_id, parent_tax_id, rank, depth;
    uint64_t direct, clade;
} mtsv_clade_stats; /* 32 bytes */
int mtsv_fold_lca(mtsv_fold *f, const mtsv_taxonomy *tx, uint32_t edit_slack, mtsv_fold *out, mtsv_clade_stats **rows,
                  uint64_t *n_rows, uint64_t *total_reads, float *device_ms);
int mtsv_format_clade_report(const mtsv_clade_stats *rows, uint64_t n_rows, uint64_t total_reads, const mtsv_taxonomy *tx,
                             char **out, uint64_t *out_len);

/* ---- abundance: how much of each taxon, by expectation-maximisation over the ambiguous reads (abund.hip, k_abund.hip) -------
 * The taxa report counts a read with twelve tied taxa twelve times and the LCA moves it to a genus or the root.
 * mtsv_fold_abundance shares every read among its taxa in proportion to (current abundance of the taxon) x (how well the read
 * fits it), re-estimates the abundances from the shares, and repeats -- the EM of Pathoscope, Bracken and Centrifuge.  The
 * definition is exact, and integer wherever an order of operations could matter, so every tier and tile gives the same bits
 * and a plain restatement with Python's int and float reproduces them (tests/abund_ref.py).
 *
 * Inputs: a fold f of any grain (N = its n_reads, U its TaxID union); a weight table w[0 .. n_w) of uint32_t in units of 2^-32,
 * 1 <= n_w <= 255; edit_slack; max_iters; tol.
 * Entries.  For a read r with records, e(r,t) is the smallest edit among r's records with TaxID t (the wide grains repeat a
 *   TaxID), m(r) the smallest edit of all r's records, d(r,t) = e(r,t) - m(r).  t ENTERS r when d <= edit_slack (0xffffffff:
 *   all, as in mtsv_fold_lca).  W(0) = 2^32 and W(d) = w[min(d, n_w) - 1] for d >= 1: the weight of the difference to the
 *   read's best, which leaves the shares as the edit itself would and keeps the best taxon's weight at exactly 1.
 * Mass.  A_k[t] is a uint64_t in units of 2^-32 reads.  A_0[t] = S for every TaxID that enters some read; S = 2^32 (one read)
 *   unless MTSV_ABUND_START_MASS (tests; 1 .. 2^32, read by mtsv_fold_create) says otherwise.
 * One iteration, for every read r and every entering t:
 *   1. x_t = (A_k[t] * W(d)) >> 48, a 128-bit product            (on the device: A >> 16 for d = 0, else
 *                                                                  __umul64hi(A, (uint64_t)W << 32) >> 16)
 *   2. s = the sum of x_t, an integer: the order of the additions does not matter
 *   3. if s == 0: x_t = W(d) >> 17 and s their sum -- the shares of a uniform prior; d = 0 makes that s >= 2^15
 *   4. q_t = (uint64_t)(((double)x_t / (double)s) * 4294967296.0): an IEEE double division, a multiplication by a power of
 *      two, a truncation.  x_t < 2^47 converts exactly; s < 2^63 is rounded once by the conversion
 *   5. A_{k+1}[t] += q_t, an integer add: the order of the adds does not matter
 *   Floating point is used only in step 4, per element (the library is built with -ffp-contract=off and without fast-math).
 * Stopping.  After iteration k + 1, L1 = sum over t of |A_{k+1}[t] - A_k[t]|; the loop stops when L1 <= tol or after max_iters
 *   iterations.  The check is made after every iteration, so the number of iterations is part of the result.  max_iters = 0
 *   is legal: A stays A_0, and the assignment below is by smallest edit.
 * Hard assignment, under the final A: read r is ASSIGNED to the entering t with the largest x_t (the fallback of step 3
 *   included), ties to the smallest TaxID as unsigned; its record is (r, t, e(r,t)).
 * Limits, both MTSV_E_LIMIT before anything is written: 2^31 or more reads with a record (keeps A below 2^63); a read with
 *   65536 or more entering taxa (keeps s below 2^63).
 * Example.  Records (read, tax, edit) (0,5,0) (1,5,1) (1,7,1) (2,5,2) (2,7,0) (3,9,3), w = {2^31, 2^30, ...}, slack all, tol 0:
 *   after iteration 1  A[5] = 7301444403  A[7] = 5583457484  A[9] = 4294967296  L1 = 4294967295
 *   after iteration 2  A[5] = 7786955038  A[7] = 5097946848  A[9] = 4294967296  L1 = 971021271
 *   after iteration 3  A[5] = 8077478865  A[7] = 4807423021  A[9] = 4294967296  L1 = 581047654
 *   and then reads 0, 1 go to TaxID 5, read 2 to 7, read 3 to 9; total_mass 17179869182.
 *
 * mtsv_fold_abundance: f is never changed.  Any of rows, info, out may be NULL; rows needs n_rows.
 *   rows: one row per TaxID that enters at least one read, ascending tax_id; malloc'd, mtsv_free.  mass = the final A;
 *     reads_any = the reads the taxon enters; reads_unique = those where it is the only one entering; assigned = the reads of
 *     the hard assignment.
 *   info: reads = the reads with a record; entries = the sum of entering taxa over reads; taxa = the rows; total_mass = the
 *     sum of mass; l1_change = the last L1 (0 with zero iterations); iterations; converged = 1 when the loop stopped on tol.
 *   out: another fold of the same device at MTSV_GRAIN_TAXID.  It becomes a fold as after mtsv_fold_reset(out, N) that holds
 *     the assigned records, its union the TaxIDs present, exactly as mtsv_fold_lca fills its out; everything a fold offers
 *     then works on it.
 *   device_ms (may be NULL): device time of the kernels.
 * MTSV_E_ARG, with both folds as they were: a null f or w; n_w outside 1..255; rows without n_rows; out == f; out on another
 *   device or of a wide grain.  An empty f gives zero rows, a zeroed info, an empty out, and no launch.  A record whose TaxID is
 *   not in f's union is an internal error, MTSV_E_DEVICE.  A refused device allocation leaves both folds as they were
 *   (MTSV_ALLOC_REFUSE names: "the abundance entries", "the abundance masses").
 * On the device (k_abund.hip).  Prepare, once per call, in tiles of MTSV_ABUND_TILE records (a power of two, 64..1024): the
 *   records become a compact entry list -- per read its offset; per entry the union slot, d clipped to n_w as a byte, e(r,t) --
 *   with reads_any, reads_unique and a work list of the reads of more than MTSV_ABUND_LANE_MAX entries (default 16, 0..1024;
 *   0 sends every read on).  An iteration streams about 5 bytes per entry: a persistent step kernel in which a lane takes
 *   each short read and a wavefront each listed read; the adds go to per-workgroup 64-bit counters in LDS, flushed with one
 *   global add per non-zero counter, when the union has at most MTSV_ABUND_DENSE_MAX TaxIDs (default 8192 = 64 KiB, 0..8192;
 *   0: never), else they are global 64-bit atomic adds.  A delta kernel computes L1, moves A_{k+1} to A_k and zeroes A_{k+1};
 *   the host reads 8 bytes per iteration.  A final kernel does the hard assignment in the same two tiers.  All knobs are
 *   read by mtsv_fold_create; results depend on none of them except MTSV_ABUND_START_MASS.  MTSV_ABUND_TIMING=1 prints the
 *   steps' times to stderr.
 * Not done here: mtsv-binner --fold-on-gpu, whose super-batches are separate folds (EM masses do not add across pieces);
 *   genome-length normalisation; a roll-up of masses through a taxonomy.
 * mtsv_abundance_weights (host only): x = 1.0; for d = 1 .. n_w: x = x * q, w[d - 1] = min((uint64_t)floor(x * 2^32),
 *   2^32 - 1).  MTSV_E_ARG unless 0 < q <= 1 and 1 <= n_w <= 255.
 * mtsv_format_abundance (host only): the TSV `taxid mass abundance_pct reads_any reads_unique assigned`, a header line and one
 *   line per row; mass is (double)mass / 2^32 as %.6f, abundance_pct (double)mass * 100 / (double)max(total_mass, 1) as %.4f.
 *   *out malloc'd, mtsv_free. */
typedef struct {
    uint32_t tax_id, _pad;
    uint64_t mass, reads_any, reads_unique, assigned;
} mtsv_abundance_row; /* 40 bytes */
typedef struct {
    uint64_t reads, entries, taxa, total_mass, l1_change;
    uint32_t iterations, converged;
} mtsv_abundance_info; /* 48 bytes */
int mtsv_fold_abundance(mtsv_fold *f, const uint32_t *w, uint32_t n_w, uint32_t edit_slack, uint32_t max_iters, uint64_t tol,
                        mtsv_fold *out, mtsv_abundance_row **rows, uint64_t *n_rows, mtsv_abundance_info *info, float *device_ms);
int mtsv_abundance_weights(double q, uint32_t n_w, uint32_t *w);
int mtsv_format_abundance(const mtsv_abundance_row *rows, uint64_t n_rows, const mtsv_abundance_info *info, char **out,
                          uint64_t *out_len);

/* ---- paired-end reads: the mates' assignments joined (pair.hip, k_pair.hip) ------------------------------------------------
 * The two mates of a fragment come from one organism, and from one reference sequence a few hundred bases apart.  A fold whose
 * reads are numbered so that reads 2p and 2p + 1 are the mates of pair p (mate 0 and mate 1) is joined into a fold of PAIRS:
 * records (p, tax_id, edit) in key order, in `out`.
 *
 * mtsv_fold_pair: f's n_reads is 2P (an odd n_reads is MTSV_E_ARG); any grain; f is not changed.  out: another fold of the
 *   same device at MTSV_GRAIN_TAXID.  It becomes a fold as after mtsv_fold_reset(out, P) that holds the records below; its
 *   TaxID union is f's.  Everything a fold offers then works on it -- mtsv_fold_download, _format_text (n_reads = P, the pairs'
 *   IDs), _taxa_report, _match_flags, _lca -- counting pairs where it counted reads.
 *   All fields compare as unsigned.  m_k(t) is the smallest edit among mate k's records with TaxID t.
 *     MTSV_PAIR_BOTH    t is kept for pair p when both mates have a record with t; its edit is m_0(t) + m_1(t).
 *     MTSV_PAIR_EITHER  the union of the mates' taxa: a taxon both mates hit carries the sum, a taxon one mate hit carries that
 *                       mate's m_k(t) + unpaired_edits, the caller's price for a mate that did not align (ignored in the other
 *                       modes; 2^31 or more is MTSV_E_ARG, so that no sum wraps).
 *     MTSV_PAIR_PROPER  f must be at MTSV_GRAIN_LONG (any other grain is MTSV_E_ARG).  t is kept when a record a of mate 0 and
 *                       a record b of mate 1 exist with equal (tax_id, gi) and |a.offset - b.offset| <= max_insert; its edit is
 *                       the smallest a.edit + b.edit over all such couples -- which need not hold the best record of either
 *                       mate.  The window [a.offset - max_insert, a.offset + max_insert] is clamped to [0, 2^32 - 1] and never
 *                       wraps.  Offsets are forward-strand window starts whichever strand hit (mtsv_hit.offset), so the
 *                       distance needs no strand; the mates' ORIENTATION (forward-reverse) is NOT checked: the records carry
 *                       no strand.  max_insert is ignored in the other two modes.
 *   stats (may be NULL), counted on the device: pairs = P; both_mates_hit / one_mate_hit: the pairs of which both mates /
 *   exactly one mate have a record in f; joined: the pairs with a record in out; records: the records of out.
 *   device_ms (may be NULL): device time of all kernels of the call.
 * On the device (k_pair.hip): the first record of every read by a lower bound; a lane per record of f that finds its window in
 *   the other mate's stretch by binary searches and walks a window of up to MTSV_PAIR_LANE_MAX records (default 16, 0..1024;
 *   0 sends every window that is not empty on) -- a longer window goes to a work list that a wavefront per entry strides; then
 *   the heads of the (read, tax_id) runs, a segmented minimum, a scan and a compaction in tiles of MTSV_PAIR_TILE records (a
 *   power of two, 64..1024); in MTSV_PAIR_EITHER the taxa only mate 1 hit form a second list that the fold's merge (k_fold.hip)
 *   joins with the first.  Both knobs are read by mtsv_fold_create (tests); results depend on neither.  MTSV_PAIR_TIMING=1
 *   prints the steps' times to stderr.  With no call made nothing is allocated or launched.  The call's arrays, kept by f, take
 *   up to 36 bytes per record of f, 4 per read, and in MTSV_PAIR_EITHER 16 per output record.
 * Refusals, all with out as it was.  MTSV_E_ARG: a null f or out; out == f; out on another device; out of a wide grain; a bad
 *   mode; an odd n_reads; MTSV_PAIR_PROPER on a narrow grain; a record of f with edit >= 2^31 (counted on the device before
 *   anything is written; no fold the library makes holds one, and it keeps the sums and the "none" sentinel apart).
 *   MTSV_E_LIMIT: 2^32 or more output records; an f of 2^32 reads or more. */
#define MTSV_PAIR_BOTH 0
#define MTSV_PAIR_EITHER 1
#define MTSV_PAIR_PROPER 2
typedef struct {
    uint64_t pairs, both_mates_hit, one_mate_hit, joined, records;
} mtsv_pair_stats; /* 40 bytes */
int mtsv_fold_pair(mtsv_fold *f, int mode, uint32_t max_insert, uint32_t unpaired_edits, mtsv_fold *out, mtsv_pair_stats *stats,
                   float *device_ms);

/* ---- coverage per reference sequence: breadth and depth (cover.hip, k_cover.hip) ---------------------------------------------
 * Everything above is counted per read.  An mtsv_coverage counts per reference POSITION: of every reference sequence how many
 * reads and alignments it took, how many bases they span and how many of its positions at least one of them covers -- what
 * tells a genome that is present (alignments all over it) from a conserved or contaminated stretch (a pile on 300 bases).
 *
 * A REFERENCE is a (tax_id, gi) with a length L, the end - start of its bin in an index.  The accumulator holds the table of
 * references, ascending by (tax_id, gi) as unsigned; the same (tax_id, gi) given twice, in one index or in two chunks, is one
 * reference with the larger L.  It is fed from folds at MTSV_GRAIN_LONG, which hold one (read, tax_id, gi, offset, edit) per
 * alignment.  For a fold f, with read_len[n_reads] the reads' lengths in the caller's numbering (as at mtsv_fold_reset):
 *   m is a read's smallest edit over all its records in f; a record COUNTS when edit <= m + edit_slack, the sum saturating as
 *   in mtsv_fold_lca (0: the best alignments only; 0xffffffff: all).  A counted record (r, t, g, o, e) covers the interval
 *   [o, min(o + read_len[r], L(t, g))) of reference (t, g).  Per reference, over every add_fold since the last reset:
 *     alignments     the counted records
 *     reads          the (read, tax_id, gi) runs of f that hold at least one counted record.  The reads of different calls are
 *                    different reads: that is the caller's contract, as with reports of several folds
 *     aligned_bases  the sum of the intervals' lengths
 *     covered_bases  the positions of the reference that lie in at least one interval, of any call
 *   All are 64-bit and exact; f is never changed.
 *   `offset` is the forward-strand start of the accepted WINDOW, not of the match (mtsv_hit.offset): the match's start less up to
 *   floor(edit_rate * read length) bases, cut at the bin's start.  An interval is therefore the read's footprint shifted left by
 *   at most that much.  Over a genome the shift is immaterial for breadth; it is documented, not corrected.
 *
 * mtsv_coverage_create: an accumulator bound to a device, with an empty table; MTSV_COVER_TILE, MTSV_COVER_LANE_MAX, MTSV_TRACE
 *   and MTSV_COVER_TIMING are read here.  Nothing but a stream is made on the device.
 * mtsv_coverage_add_index: the bins' (tax_id, gi, end - start) of a loaded index join the table.  Host only: the index need
 *   not be resident, and may be freed afterwards.  mtsv_coverage_add_refs: the same from arrays.
 *   References are fixed once alignments exist: they may be added until the first add_fold after a create or reset that
 *   is not refused (a fold without records counts; a refused call leaves the accumulator as it was, the open table
 *   included).  After that, a call that brings a NEW reference or a LONGER length is MTSV_E_ARG and
 *   changes nothing; one that brings only what the table holds (equal or shorter lengths) is accepted and does nothing --
 *   mtsv-binner adds every chunk once per super-batch.
 * mtsv_coverage_reset: counters and bitmap zero, the table stays and may grow again.
 * mtsv_coverage_add_fold: as above.  device_ms (may be NULL): device time of the kernels.  A fold without records returns at
 *   once: nothing is launched, *device_ms is 0.
 * mtsv_coverage_rows: EVERY reference of the table, hit or not, ascending by (tax_id, gi): malloc'd, mtsv_free.  Before the
 *   first add_fold nothing is launched.  The accumulator is not changed and goes on accumulating.
 * mtsv_format_coverage_report (host only, needs no device): the TSV
 *     taxid gi length reads alignments aligned_bases depth covered_bases breadth_pct
 *   one line per reference with alignments > 0, in the rows' order; depth = aligned_bases / length, breadth_pct =
 *   covered_bases / length * 100, both %.2f of doubles; a length of 0 prints 0.00 for both.  After the references of a TaxID
 *   that has any such line, one ROLLUP line: gi is `*`, length sums ALL the taxon's references, hit or not (which is why rows
 *   returns them all), the counters are summed, depth and breadth_pct are taken of the sums.  A taxon without a hit prints
 *   nothing.
 * On the device (k_cover.hip), on a stream of the accumulator's own.  The bitmap gives every reference a whole number of 64-bit
 *   words, so that no word belongs to two references; it is laid out, with the table, by the first add_fold.  add_fold: the
 *   first record of every read by a lower bound; the reads' smallest edits, a lane per read and the wavefront for a read of
 *   more than 32 records; a lane per record that decides whether it counts, finds its reference by binary search and flags the
 *   heads of the runs -- here the host reads the counters and refuses; then a lane per counted record ORs its interval into
 *   the bitmap when it spans up to MTSV_COVER_LANE_MAX words (default 8, 0..1024; 0 sends every interval that is not empty on),
 *   a longer one goes to a work list that a wavefront per entry strides; a word that holds the mask already is not written
 *   again; the counters are combined per wavefront and reference before they are added.  rows: the bitmap is popcounted in
 *   tiles of MTSV_COVER_TILE words (a power of two, 64..1024).  Every atomic is an integer OR or add: results are exact and do
 *   not depend on either knob or on the order of execution.  Memory: 8 bytes per 64 bases of the table and 48 per reference,
 *   and per call 24 bytes per record and 12 per read, kept.
 * Refusals of add_fold, each leaving the accumulator byte for byte as it was.  MTSV_E_ARG: a null handle or read_len; f not at
 *   MTSV_GRAIN_LONG; f on another device; n_reads not the fold's; a record whose (tax_id, gi) the table does not hold; a record
 *   whose offset is L or more -- these two are counted on the device in a pass of its own before anything is marked or added,
 *   and mtsv_last_error gives the counts and names the first such record.  MTSV_E_LIMIT: a fold of 2^32 reads or more.
 *   MTSV_E_LIMIT of add_index / add_refs, the table as it was: a length of 2^32 or more; a table whose bitmap would take 2^32
 *   words or more. */
typedef struct mtsv_coverage mtsv_coverage;
typedef struct {
    uint32_t tax_id, gi;
    uint64_t length, reads, alignments, aligned_bases, covered_bases;
} mtsv_ref_coverage; /* 48 bytes */
int mtsv_coverage_create(int hip_device, mtsv_coverage **out);
void mtsv_coverage_free(mtsv_coverage *c);
int mtsv_coverage_add_index(mtsv_coverage *c, const mtsv_index *ix);
int mtsv_coverage_add_refs(mtsv_coverage *c, const uint32_t *tax_id, const uint32_t *gi, const uint64_t *length, uint64_t n);
int mtsv_coverage_reset(mtsv_coverage *c);
int mtsv_coverage_add_fold(mtsv_coverage *c, mtsv_fold *f, const uint32_t *read_len, uint64_t n_reads, uint32_t edit_slack,
                           float *device_ms);
int mtsv_coverage_rows(mtsv_coverage *c, mtsv_ref_coverage **rows, uint64_t *n_rows, float *device_ms);
int mtsv_format_coverage_report(const mtsv_ref_coverage *rows, uint64_t n_rows, char **out, uint64_t *out_len);

/* ---- alignments: where a hit lies in its reference, on which strand, and its edit script (place.hip, k_place.hip) -----------
 * A hit says which reference a read aligned to and with how many edits; its `offset` is the start of the accepted WINDOW.  A
 * PLACEMENT adds the alignment itself.  For one hit (read, strand, tax_id, gi, offset, edit):
 *   P is the read's codes on that strand -- forward, or reverse complement with N staying N -- and L their number; b is the bin
 *   of (tax_id, gi); T = text[b.start + offset, b.end).  Row i matches column j iff P[i-1] == T[j-1] and the code is a base: an
 *   N on either side never matches (align.rs after N -> '.').  D is the semi-global matrix of align.rs:28-85: D[0][j] = 0,
 *   D[i][0] = i, unit costs.
 *   end    the smallest j >= 0 with D[L][j] <= edit.  For a hit the binner produced that is the leftmost minimum of the
 *          window's last row; it lies inside the accepted window and does not depend on the window's end.
 *   path   from (L, end) while i > 0: the diagonal when j > 0 and D[i-1][j-1] + (match ? 0 : 1) == D[i][j] (op '=' or 'X');
 *          else the step up when D[i-1][j] + 1 == D[i][j] (op 'I': a read base and no reference base); else the step left
 *          (op 'D').  At i == 0, start = j.
 *   ref_start = offset + start, ref_end = offset + end: forward-strand offsets inside the GI, half open.  The ops are run-length
 *   encoded in reference order as len << 4 | op with BAM's codes I = 1, D = 2, '=' = 7, X = 8; at most 2 * edit + 1 runs.
 *   A hit is UNPLACEABLE when no column of T reaches its edit: only a hit a caller made up.
 * mtsv_batch_place_hits: hits == NULL places the hits of the workspace's last run where they lie in HBM -- every stretch, in the
 *   order mtsv_batch_download returns them, in any assignment mode, MTSV_ASSIGN_ONLY included; otherwise `hits` are n_hits
 *   caller-given hits, uploaded and placed against the resident batch.  It needs a resident batch (mtsv_batch_upload,
 *   _take_reads, _take_unique, _copy_reads: after the last two `read` is the caller's number, found in the read map) and, for
 *   hits == NULL, a completed mtsv_batch_run or mtsv_batch_merge_runs on it.  Placement k describes hit k; its ops are
 *   (*ops)[ops_off .. ops_off + n_ops).  The ops array is sized before the kernel runs, 2 * min(edit, L) + 1 slots per hit, and
 *   may hold unused slots between hits, which are zero: *n_ops_total is its length.  Both arrays: mtsv_free.  device_ms (may be NULL): the
 *   device time of the map pass and scan, the placement kernel and the copies to the host.  Zero hits: two empty arrays,
 *   nothing is launched.  A workspace that never calls this allocates and launches nothing for it.
 *   Nothing of the run is changed: hits, assignments, statistics, flags and report are what they were.
 *   MTSV_PLACE_RING (tests; read by the workspace's first call): columns of the ring the kernel keeps per hit, a power of two,
 *   forced up to what the call needs.  MTSV_PLACE_TIMING=1: one line per call on stderr with the steps' times.
 * Refusals, each leaving the workspace as it was; mtsv_last_error gives the counts and the first offender.  MTSV_E_ARG: null
 *   arguments; no resident batch, or a host batch; hits == NULL without such a run; an index that holds one (tax_id, gi) in two
 *   bins (checked on the host); a hit whose (tax_id, gi) the index does not hold, whose offset is at or beyond its bin's
 *   length, whose read is not resident, whose strand is above 1 (all counted on the device before anything is placed), or that
 *   is unplaceable (counted by the placement kernel, before anything is handed out).  MTSV_E_LIMIT: a resident read above 256
 *   bases; 2^32 hits or op slots or more.
 * mtsv_format_placements (host only, needs no device): one line per placement, in the order given,
 *     READ_ID \t TAXID \t GI \t +|- \t START \t END \t EDIT \t CIGAR \n
 *   CIGAR as text, e.g. 37=1X112=, `*` for a placement without ops (a read of no bases).  ids = NUL-separated read ids,
 *   id_off[n_reads + 1].  MTSV_E_ARG: a read >= n_reads. */
typedef struct {
    uint64_t read;
    uint32_t tax_id, gi, edit;
    uint8_t strand, _pad[3];
    uint32_t ref_start, ref_end, n_ops;
    uint64_t ops_off; /* (8-byte aligned: four bytes of padding lie before it) */
} mtsv_placement; /* 48 bytes */
int mtsv_batch_place_hits(mtsv_batch *b, const mtsv_hit *hits, uint64_t n_hits, mtsv_placement **out, uint64_t *n_out,
                          uint32_t **ops, uint64_t *n_ops_total, float *device_ms);
int mtsv_format_placements(const mtsv_placement *pl, uint64_t n, const uint32_t *ops, const char *ids, const uint64_t *id_off,
                           uint64_t n_reads, char **out, uint64_t *out_len);

/* ---- pileup: what the reads show at every reference position (pile.hip, k_pile.hip) ------------------------------------------
 * The alignments above are per hit.  An mtsv_pileup adds them up per reference POSITION: how many reads match there, how many
 * show an A, C, G, T or N instead, how many skip the position, and how many carry extra bases in front of it.  It is bound to a
 * device and to an optional list of TaxIDs (n_taxa == 0: every reference).
 *   A reference is a (tax_id, gi) of length L = end - start of its bin.  It owns L + 1 SLOTS: positions 0 .. L-1, and slot L,
 *   which can only take insertions (a read base behind the bin's last base).  A slot has eight u32 counters n[0 .. 8):
 *   n[0] match, n[1 .. 4] a read A, C, G, T over another base, n[5] a read N, n[6] deletion, n[7] insertion.
 *   For a hit and its placement (ref_start, the ops in reference order, as mtsv_batch_place_hits defines them) and P the read's
 *   codes on the hit's strand -- forward, or reverse complement with N staying N -- the ops are walked with i = 0, j = ref_start:
 *     a run of n '='   adds 1 to n[0] of positions j .. j+n-1; i += n, j += n
 *     each 'X'         adds 1 to n[1 + P[i]] of position j; i++, j++
 *     each 'D'         adds 1 to n[6] of position j; j++
 *     a run of n 'I'   adds 1 to n[7] of slot j, once per run; i += n
 *   depth(pos) = n[0] + ... + n[6].  ref is the text's code at the position (0 .. 4 for A, C, G, T, N); slot L has 0xff.
 *   A hit COUNTS when edit <= m + edit_slack, the sum saturating, m the smallest edit among the hits OF THIS CALL that carry the
 *   same read -- every hit of the call, also one on a reference the list does not select; a slack of 0xffffffff: all hits.  The
 *   best is per call: the binner calls once per chunk run, so a read's best there is its best in that chunk, not over the
 *   database.  A hit on a reference whose TaxID the list does not select is SKIPPED and counted in *n_skipped; *n_piled: the
 *   hits that were walked.
 * mtsv_pileup_add_run: hits == NULL piles the hits of the workspace's last run where they lie; otherwise `hits` are n_hits
 *   caller-given hits against the resident batch -- exactly as in mtsv_batch_place_hits, with its preconditions.  The hits are
 *   placed (on the workspace's stream; no placement and no op comes to the host), then walked.  References are learnt from the
 *   workspace's index at each call: the selected bins whose (tax_id, gi) the accumulator does not hold yet form a new SEGMENT
 *   with device arrays of its own -- counters, and ref codes copied from the resident text on the device; nothing that exists
 *   is reallocated.  A chunk that is loaded again, as a new handle, finds its references by key and adds no segment.  Zero hits:
 *   nothing is launched, device_ms is 0 and no reference is learnt.  device_ms (may be NULL, as n_piled and n_skipped): the
 *   device time of the placement, the best-edit pass and the pile kernel.
 *   Memory: 32 bytes of counters and one of ref code per slot, 33 bytes per reference base -- a database of 3e9 bases would
 *   take 99 GB, which is why the TaxID list exists.
 * mtsv_pileup_reset: counters and the two hit totals zero, the references and segments stay.
 * mtsv_pileup_info: n_refs references in n_slots slots of n_segments segments and device_bytes; hits_piled, hits_skipped.
 * mtsv_pileup_download (tests): one reference's counters as [slot][8] u32 and its ref codes, L + 1 slots; both malloc'd,
 *   mtsv_free.  MTSV_E_ARG for a (tax_id, gi) the accumulator does not hold.
 * mtsv_pileup_sites: a slot is a SITE when depth + n[7] > 0, depth >= min_depth, and some channel c in 1 .. 7 has
 *   n[c] >= min_alt and n[c] * 1000000 >= min_alt_ppm * depth, in 64-bit integers.  (0, 0, 0) returns every touched slot.
 *   Rows ascend by (tax_id, gi, pos) as unsigned; malloc'd, mtsv_free; the accumulator is unchanged.  device_ms (may be NULL):
 *   the device time of the kernels.
 * mtsv_format_variants (host only, needs no device): the header line
 *     taxid \t gi \t pos \t ref \t depth \t match \t A \t C \t G \t T \t N \t del \t ins
 *   then one such line per row; pos is 0-based, like START of mtsv_format_placements; ref is one of ACGTN, or `.` for slot L.
 * On the device (k_pile.hip): channel 0 is a difference array -- a run of '=' adds +1 at its first position and -1 at the slot
 *   behind its last, which lies in the same reference because slot L exists -- so a clean read costs two atomics; sites and
 *   download integrate it, per tile of MTSV_PILE_TILE slots (tests; a power of two, 64 .. 1024, read at create) with the prefix
 *   carried from tile to tile.  Every atomic is an integer add or min: the counters are exact and depend on neither the tile
 *   nor the order of execution.  MTSV_PILE_TIMING=1: one line per add_run and sites on stderr with the steps' times.
 * Refusals of add_run, each leaving the accumulator byte for byte as it was, no segment added and no counter changed:
 *   everything mtsv_batch_place_hits refuses, with its codes and texts (a read above 256 bases, an unknown (tax_id, gi), an
 *   offset beyond the bin, a read that is not resident, a strand above 1, an unplaceable hit, a host batch, no completed run).
 *   MTSV_E_ARG: a null handle; a workspace on another device; a (tax_id, gi) the accumulator holds with another length.
 *   MTSV_E_LIMIT: a segment of 2^32 slots or more; a total of piled hits that would reach 2^32 (the counters are 32 bits).
 *   MTSV_E_NOMEM: a segment the device has no room for ("the pileup segment" for MTSV_ALLOC_REFUSE). */
typedef struct mtsv_pileup mtsv_pileup;
typedef struct {
    uint32_t tax_id, gi, pos;
    uint8_t ref, _pad[3];
    uint32_t n[8];
} mtsv_pile_site; /* 48 bytes */
typedef struct {
    uint64_t n_refs, n_slots, n_segments, device_bytes, hits_piled, hits_skipped;
} mtsv_pileup_info_t;
int mtsv_pileup_create(int hip_device, const uint32_t *taxa, uint64_t n_taxa, mtsv_pileup **out);
void mtsv_pileup_free(mtsv_pileup *p);
int mtsv_pileup_reset(mtsv_pileup *p);
int mtsv_pileup_add_run(mtsv_pileup *p, mtsv_batch *b, const mtsv_hit *hits, uint64_t n_hits, uint32_t edit_slack,
                        uint64_t *n_piled, uint64_t *n_skipped, float *device_ms);
int mtsv_pileup_info(const mtsv_pileup *p, mtsv_pileup_info_t *info);
int mtsv_pileup_download(mtsv_pileup *p, uint32_t tax_id, uint32_t gi, uint32_t **counts, uint8_t **ref, uint64_t *n_slots);
int mtsv_pileup_sites(mtsv_pileup *p, uint32_t min_depth, uint32_t min_alt, uint32_t min_alt_ppm, mtsv_pile_site **rows,
                      uint64_t *n_rows, float *device_ms);
int mtsv_format_variants(const mtsv_pile_site *rows, uint64_t n_rows, char **out, uint64_t *out_len);

/* ---- consensus: a sequence and call statistics per reference from the pileup (cons.hip, k_cons.hip) ------------------------
 * What the organism in the sample looks like, and how close it is to the database entry: a consensus sequence per reference as
 * FASTA, written on the device (about one byte per base crosses to the host), and one row of call statistics per reference.
 * Parameters: min_depth, min_frac_ppm, min_breadth_ppm, fill (0 = `N`, 1 = the reference base in lower case), line_width
 * (0 = no wrapping).  Let md = max(min_depth, 1).
 *   The counters of a slot are the integrated n[0 .. 8) that mtsv_pileup_download shows.  For position p in 0 .. L-1 of a
 *   reference: depth = n[0] + ... + n[6]; w is the channel in 0 .. 6 with the largest count, the lowest channel on equal
 *   counts, so match wins a tie.  Each position falls into exactly one class:
 *     LOW    depth < md                                                              emits the fill character
 *     AMBIG  depth >= md and (w == 5, a read N, or n[w] * 1000000 < min_frac_ppm * depth in 64-bit integers)
 *                                                                                    emits the fill character
 *     REF    w == 0, otherwise         emits the reference base in upper case (ACGTN by ref code)
 *     SUB    w in 1 .. 4, otherwise    emits ACGT[w - 1]
 *     DEL    w == 6, otherwise         emits nothing
 *   The fill character is `N` for fill == 0 and the reference base in lower case (acgtn) for fill == 1.
 *   INSERTIONS CANNOT BE SPELLED: the pileup keeps how many reads insert in front of a slot, not which bases.  They are only
 *   counted: slot j in 0 .. L is an INS SITE when n[7] >= md and 2 * n[7] > D, D = depth(j) for j < L and 0 for slot L.  The
 *   consensus text never holds an inserted base.
 *   The row of a reference, mtsv_cons_ref: covered counts the positions with depth >= md, sum_depth sums depth over the
 *   positions, n_ref .. n_ambig count the classes, ins_sites the INS SITES.  length = covered + n_low and
 *   covered = n_ref + n_sub + n_del + n_ambig.  cons_len = length - n_del.
 *   A reference is EMITTED when covered >= 1 and covered * 1000000 >= min_breadth_ppm * length.  Rows and sequences are those
 *   of the emitted references, ascending by (tax_id, gi) as unsigned, across segments.
 *   FASTA for each emitted reference: `>` GI `-` TAXID `\n` (the header form mtsv-build reads), then the cons_len characters
 *   in lines of line_width, the last line shorter, every line ended by `\n`; no empty line when cons_len is a multiple of the
 *   width; the header line alone when cons_len == 0; one line when line_width == 0.
 * mtsv_pileup_consensus: fasta == NULL gives rows only, and no layout or write kernel is launched; rows (with n_rows) may be
 *   NULL too.  *fasta (fasta_len bytes, not terminated) and *rows are malloc'd, mtsv_free.  The accumulator is unchanged.  An
 *   accumulator without segments returns empty text, zero rows and device_ms 0 without a launch.  device_ms (may be NULL): the
 *   device time of the call pass, the layout and the write pass.  MTSV_PILE_TIMING=1: one line on stderr with the steps' times.
 *   MTSV_E_ARG: fill > 1, min_frac_ppm > 1000000, a null handle.  MTSV_E_LIMIT: a segment whose text would reach 2^32 bytes.
 *   MTSV_E_NOMEM: "the consensus calls", "the consensus text" (names for MTSV_ALLOC_REFUSE).  Each refusal leaves the
 *   accumulator as it was.
 * mtsv_format_consensus_stats (host only, needs no device): the header line
 *     taxid gi length covered breadth_pct mean_depth cons_len ref sub del low ambiguous ins_sites identity_pct
 *   (tab-separated), a line per row, and after a TaxID's rows one rollup line with gi `*` that takes the sums of that taxon's
 *   rows, the three ratios taken of the sums.  breadth_pct = covered / length * 100, mean_depth = sum_depth / length,
 *   identity_pct = ref / (ref + sub + del) * 100, each %.2f of doubles and 0.00 on a zero denominator.
 * mtsv_pileup_add_counts: adds caller-given counts, [n_slots][8] u32, plain as mtsv_pileup_download gives them, to slots
 *   first_slot .. first_slot + n_slots - 1 of a reference the accumulator already holds, by a kernel on the accumulator's
 *   stream (channel 0 goes into the difference form); n_hits is added to hits_piled.  Pileups made on several nodes or days
 *   are merged so before the consensus is called.  MTSV_E_ARG, the accumulator unchanged: any count above n_hits (with the
 *   limit below, no counter can overflow); an unknown reference; a range beyond L + 1 slots; a nonzero channel 0 .. 6 in
 *   slot L.  MTSV_E_LIMIT: a total of piled hits that would reach 2^32. */
typedef struct {
    uint32_t tax_id, gi, length, covered, n_ref, n_sub, n_del, n_low, n_ambig, ins_sites;
    uint64_t sum_depth;
} mtsv_cons_ref; /* 48 bytes */
int mtsv_pileup_consensus(mtsv_pileup *p, uint32_t min_depth, uint32_t min_frac_ppm, uint32_t min_breadth_ppm, uint32_t fill,
                          uint32_t line_width, char **fasta, uint64_t *fasta_len, mtsv_cons_ref **rows, uint64_t *n_rows,
                          float *device_ms);
int mtsv_format_consensus_stats(const mtsv_cons_ref *rows, uint64_t n_rows, char **out, uint64_t *out_len);
int mtsv_pileup_add_counts(mtsv_pileup *p, uint32_t tax_id, uint32_t gi, uint32_t first_slot, uint64_t n_slots,
                           const uint32_t *counts, uint64_t n_hits);

/* ---- result lines (host) ---------------------------------------------------------------- */
/* write_assignments for a whole batch: hits ordered by read; ids = NUL-separated read ids,
 * id_off[n_reads+1].  Lines are appended to a malloc'd buffer (*out, *out_len), one per read with
 * >= 1 hit, in read order.  long_format = --output-format long. */
int mtsv_format_results(const mtsv_hit *hits, uint64_t n_hits, const char *ids,
                        const uint64_t *id_off, uint64_t n_reads, int long_format, char **out,
                        uint64_t *out_len);
/* The same lines from assignments (mtsv_batch_download_assignments): one per read that has any, READ_ID:TAXID=EDIT,...
 * in the order given -- nothing is de-duplicated or sorted here.  Byte-identical to mtsv_format_results(long_format = 0)
 * on the hits of the same run.  MTSV_E_ARG: reads not in ascending order, a read >= n_reads.  Host only, needs no device. */
int mtsv_format_assignments(const mtsv_assignment *a, uint64_t n, const char *ids, const uint64_t *id_off,
                            uint64_t n_reads, char **out, uint64_t *out_len);
/* READ_ID:TAXID-GI-OFFSET=EDIT,... from wide assignments (mtsv_batch_download_assignments_gi), one line per read that has
 * any, in the order given: nothing is sorted or de-duplicated.  On MTSV_GRAIN_LONG records byte-identical to
 * mtsv_format_results(long_format = 1) on the hits of the same run.  MTSV_E_ARG: reads not in ascending order, a read
 * >= n_reads.  Host only, needs no device. */
int mtsv_format_assignments_gi(const mtsv_assignment_gi *a, uint64_t n, const char *ids, const uint64_t *id_off,
                               uint64_t n_reads, char **out, uint64_t *out_len);
/* frees what the library malloc'd, and returns arrays of its page-locked pool (mtsv_batch_download_assignments) to it */
void mtsv_free(void *p);

/* ---- the transfer format of mtsv_batch_run_host*, exposed for tests (not part of the drop-in) ---- */
/* The bases of a host batch cross PCIe as 4-bit codes, two per byte (src/binner.rs:88-100 applied on the host: A/a C/c
 * G/g T/t -> 0..3, any other byte -> 4): src[0, n) are the bases at offsets [first_offset, first_offset + n) of a segment,
 * dst receives bytes [first_offset / 2, (first_offset + n + 1) / 2) of its packed image (base i in nibble i & 1 of byte
 * i / 2); prev_code is the code of the base before the first (it shares the first byte when first_offset is odd).
 * Returns the code of the last base. */
uint8_t mtsv_pack_bases(uint8_t *dst, const uint8_t *src, uint64_t first_offset, uint64_t n, uint8_t prev_code);
/* Host threads that pack the bases of a host batch in this process (the CPUs it may use less four, ten at most;
 * MTSV_PACK_THREADS overrides); 0: the bytes go as they are (MTSV_H2D_PLAIN=1, or fewer than nine threads). */
int mtsv_host_pack_threads(void);

/* ---- synthetic workloads for bench.py / tests (not part of the drop-in) ---- */
/* i.i.d. ACGT reference of n_taxa x gis_per_taxon sequences of seq_len, 5% of each overwritten by
 * a 1%-diverged copy from another taxon, 0.1% of positions in N runs; built straight into an index */
int mtsv_synth_index(uint64_t seed, uint32_t n_taxa, uint32_t gis_per_taxon, uint64_t seq_len,
                     uint32_t occ_k, uint64_t sa_s, int n_threads, mtsv_index **out);
/* n_reads reads of read_len sampled from the index text (90%: sub 1%, ins 0.1%, del 0.1%, N 0.2%,
 * half reverse-complemented; 10% random).  bases must hold n_reads*read_len bytes. */
int mtsv_synth_reads(const mtsv_index *ix, uint64_t seed, uint64_t n_reads, uint32_t read_len,
                     uint8_t *bases, uint64_t *read_off);

#ifdef __cplusplus
}
#endif
#endif /* MTSV_AMD_H */
