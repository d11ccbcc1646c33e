/*
 * chromap_amd.h -- C ABI of the MI355X (gfx950) implementation of Chromap's per-read
 * mapping hot path.
 *
 * The reference (haowenz/chromap v0.3.3, /root/reference) has no plugin or FFI seam; the
 * replacement point is the body of the per-batch OpenMP taskloop in
 * Chromap::MapPairedEndReads (src/chromap.h:892-1143) together with the one-time loads in
 * front of it (src/chromap.h:641-670).  Each entry point below names the reference
 * code it stands in for.  Plain pointers and sizes only; no C++ or torch types.
 *
 * All functions return 0 on success and a negative CMGPU_E* code on failure; the text of
 * the last failure is available from cmgpu_last_error().  The reference's convention is
 * to abort the process (ExitWithMessage -> exit(-1), src/utils.h:71-74); the host driver
 * turns a non-zero status into exactly that.  There is no CPU fallback: without a HIP
 * device cmgpu_create fails with CMGPU_ENODEVICE.
 */
#ifndef CHROMAP_AMD_H_
#define CHROMAP_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMGPU_OK 0
#define CMGPU_EINVAL (-1)
#define CMGPU_ENODEVICE (-2)
#define CMGPU_EHIP (-3)
#define CMGPU_ENOMEM (-4)
#define CMGPU_ECAPACITY (-5)
#define CMGPU_EIO (-6)
#define CMGPU_EFORMAT (-7)

#define CMGPU_FORMAT_SAM 1
#define CMGPU_FORMAT_PAIRS 2 /* --pairs WITHOUT split alignment: cmgpu_map_pairs leaves cmgpu_pairs_record entries (MapPairedEndReads<PairsMapping>, src/chromap_driver.cc:748-751) */

/* The minimizer index exactly as Index::Load leaves it in host memory
 * (src/index.cc:132-169, kh_load src/khash.h:358-373): khash open-addressing arrays with
 * 2-bit flags, keys = minimizer_hash<<1 | is_singleton, values, and the occurrence
 * table.  The library re-packs it for HBM; the caller keeps ownership. */
typedef struct cmgpu_index_view {
  int32_t kmer_size;   /* Index::kmer_size_, read from the index file */
  int32_t window_size; /* Index::window_size_ */
  uint32_t n_buckets;  /* kh_n_buckets, a power of two */
  const uint32_t *flags; /* n_buckets/16 words (at least 1) */
  const uint64_t *keys;  /* n_buckets */
  const uint64_t *vals;  /* n_buckets */
  uint32_t n_occurrences;
  const uint64_t *occurrences;
} cmgpu_index_view;

/* The reference sequences as SequenceBatch::LoadAllSequences holds them
 * (src/sequence_batch.cc:84-120): raw bytes, case and N preserved, file order. */
typedef struct cmgpu_ref_view {
  uint32_t n_sequences;
  const char *const *names;     /* used only by cmgpu_write_bed_pe */
  const char *const *sequences; /* n_sequences pointers, lengths[] bytes each */
  const uint32_t *lengths;
} cmgpu_ref_view;

/* The fields of MappingParameters the path reads (src/mapping_parameters.h:18-89). */
typedef struct cmgpu_params {
  int32_t error_threshold;        /* -e */
  int32_t min_num_seeds;          /* -s */
  int32_t max_seed_frequency0;    /* -f first value */
  int32_t max_seed_frequency1;    /* -f second value */
  int32_t max_insert_size;        /* -l */
  int32_t min_read_length;        /* --min-read-length */
  int32_t max_num_best_mappings;  /* -n: up to this many records per read / pair (1..8192), reservoir-sampled when there are more
                                   * best mappings (mapping_generator.h:121-139,199-214); not with CMGPU_FORMAT_SAM */
  int32_t drop_repetitive_reads;  /* --drop-repetitive-reads */
  int32_t trim_adapters;          /* --trim-adapters */
  int32_t split_alignment;        /* --split-alignment: paired-end batches leave cmgpu_pairs_record entries; single-end batches (cmgpu_map_single,
                                   * cmgpu_map_single_barcoded, a single-end cmgpu_fastq_commit) leave ordinary cmgpu_record entries whose coordinates
                                   * and MAPQ carry the read's split site */
  int32_t mapq_threshold;         /* -q; used by cmgpu_write_bed_pe only */
  int32_t remove_pcr_duplicates;  /* used by the writers / cmgpu_store_format* only */
  int32_t tn5_shift;              /* used by cmgpu_write_bed_pe only */
  int32_t low_memory_mode;        /* used by the writers / cmgpu_store_format* only */
  int32_t read_batch_size;        /* Chromap::read_batch_size_ = 500000 (chromap.h:182) */
  int32_t taskloop_grain_size;    /* 5000 (chromap.h:887): scope of the reservoir RNG */
  int32_t bc_error_threshold;     /* --bc-error-threshold (0, 1 or 2 on the device) */
  int32_t output_mappings_not_in_whitelist; /* --output-mappings-not-in-whitelist */
  int32_t output_format;          /* 0: BED records (pairs records for paired-end batches with split_alignment); CMGPU_FORMAT_SAM: --SAM (alignment coordinates, CIGAR,
                                   * NM, MD); CMGPU_FORMAT_PAIRS: pairs records from the ordinary (non-split) pairing */
  int32_t dedup_at_bulk_level;    /* single-cell BED, low-memory flavour: --remove-pcr-duplicates-at-bulk-level (the reference's
                                   * default without --preset atac); applied by cmgpu_store_format only */
  int32_t allocate_multi_mappings; /* --allocate-multi-mappings: in-memory flavour only (low_memory_mode == 0); cmgpu_store_format of the BED /
                                    * TagAlign kinds, cmgpu_write_bed_pe / _se / _pe_bc */
  int32_t multi_mapping_allocation_distance; /* --multi-mapping-allocation-distance (0) */
  int32_t multi_mapping_allocation_seed;     /* --multi-mapping-allocation-seed (11) */
  double bc_probability_threshold; /* --bc-probability-threshold */
} cmgpu_params;

/* A batch of read pairs as SequenceBatch holds them after parsing (src/chromap.cc:93-174):
 * concatenated ASCII bases (any case, N allowed) with n+1 offsets per mate.  read_id of
 * pair i is first_read_id + i (src/sequence_batch.cc:38-39). */
typedef struct cmgpu_batch {
  uint32_t n_pairs;
  uint32_t first_read_id;
  const char *read1_bases;
  const uint32_t *read1_offsets; /* n_pairs + 1 */
  const char *read2_bases;
  const uint32_t *read2_offsets; /* n_pairs + 1 */
} cmgpu_batch;

/* Constructor arguments of PairedEndMappingWithoutBarcode (src/bed_mapping.h:191-206) plus
 * rid, which the reference keeps implicitly as the index of the per-chromosome vector
 * (src/mapping_generator.cc:116). 24 bytes. */
typedef struct cmgpu_record {
  uint32_t read_id;
  uint32_t rid;
  uint32_t fragment_start;
  uint16_t fragment_length;
  uint8_t mapq;      /* 6-bit field in the reference */
  uint8_t direction; /* 1: read1 maps to the + strand */
  uint8_t is_unique;
  uint8_t num_dups;  /* 1 */
  uint16_t positive_alignment_length;
  uint16_t negative_alignment_length;
} cmgpu_record;

/* With params.split_alignment (--preset hic) the record of a PAIRED-END batch is the constructor argument list of
 * PairsMapping (src/pairs_mapping.h:25-38) without read name and barcode, already flipped so
 * that (rid1,pos1) <= (rid2,pos2) (src/mapping_generator.cc:169-210); pos = ref start for a +
 * read, ref end for a - read, 0-based.  Same 24-byte slot as cmgpu_record: the `out` buffers of
 * cmgpu_map_pairs / cmgpu_download_records then hold cmgpu_pairs_record entries.  A single-end batch of the same context
 * (cmgpu_map_single, cmgpu_map_single_barcoded) holds cmgpu_record entries: fragment_length = ref_end - ref_start + 1 of the part of the
 * read that was aligned. */
typedef struct cmgpu_pairs_record {
  uint32_t read_id;
  uint32_t rid1, rid2;
  uint32_t pos1, pos2;
  uint8_t strand1, strand2; /* 1 = positive */
  uint8_t mapq;
  uint8_t is_unique;
} cmgpu_pairs_record;

/* Single-cell data: PairedEndMappingWithBarcode (src/bed_mapping.h:128-144) = the bulk record
 * plus the 2-bit-packed (corrected) cell barcode (GenerateSeedFromSequence, src/utils.h:111-129). */
typedef struct cmgpu_record_bc {
  cmgpu_record r;
  uint64_t barcode;
} cmgpu_record_bc;

/* Cell barcodes of a batch as the barcode SequenceBatch holds them: bases + qualities
 * (same offsets), n_pairs+1 offsets. */
typedef struct cmgpu_barcode_batch {
  const char *bases;
  const char *qualities;
  const uint32_t *offsets;
} cmgpu_barcode_batch;

/* Counters of Chromap::OutputMappingStatistics (src/chromap.cc:808-823) plus the
 * quantities SURVEY.md 8(d) defines the index-probe kernel's algorithmic bytes from. */
typedef struct cmgpu_stats {
  uint64_t num_candidates;
  uint64_t num_mappings;
  uint64_t num_mapped_reads;
  uint64_t num_uniquely_mapped_reads;
  uint64_t num_minimizers;      /* lookups issued by the probe kernel */
  uint64_t probe_steps;         /* hash buckets visited by the probe kernel (16 B each) */
  uint64_t occurrences_read;    /* occurrence-table entries expanded (8 B each) */
  uint64_t num_pairs_rescued;   /* reads that went through mate rescue */
  uint64_t num_multi_mappers;   /* pairs resolved by reservoir sampling */
  uint64_t num_barcode_in_whitelist; /* Chromap::OutputBarcodeStatistics (chromap.cc:801-806) */
  uint64_t num_corrected_barcode;
  uint64_t reserved[5];
} cmgpu_stats;

typedef struct cmgpu_ctx cmgpu_ctx;

/* Fills *p with the reference's defaults (src/mapping_parameters.h:19-61). */
void cmgpu_default_params(cmgpu_params *p);
/* Applies a CLI preset ("atac", "chip", "hic") the way chromap_driver.cc:247-275 does. */
int cmgpu_apply_preset(cmgpu_params *p, const char *preset);

/* Replaces: reference.LoadAllSequences() + index.Load() + construction of the stateless
 * worker objects (src/chromap.h:641-670, 763-778).  Uploads index and reference to the
 * HBM of device_id once. */
int cmgpu_create(const cmgpu_index_view *index, const cmgpu_ref_view *ref, const cmgpu_params *params,
                 int device_id, cmgpu_ctx **out);

/* Replaces: Index::Construct (src/index.cc:12-89) -- builds the minimizer index of `ref` on
 * the device (chunked minimizer pass, radix sort by (hash, hit), khash-sized open-addressing
 * table) and keeps it resident together with the reference; the ctx maps like one made by
 * cmgpu_create.  cmgpu_save_index_file replaces Index::Save (src/index.cc:91-121): the file
 * loads in the reference (kh_load) and answers every lookup identically. */
int cmgpu_create_from_reference(const cmgpu_ref_view *ref, int32_t kmer_size, int32_t window_size,
                                const cmgpu_params *params, int device_id, cmgpu_ctx **out);
int cmgpu_save_index_file(cmgpu_ctx *ctx, const char *path);

/* --chr-order (Chromap::GenerateCustomRidRanks + SequenceBatch::ReorderSequences + RerankCandidatesRid,
 * src/chromap.cc:867-923, src/chromap.h:654-659, 1060-1074): rank[i] = place of reference sequence i in the
 * output order.  Records then carry ranks in their rid fields; pass names / lengths in rank order to the writers. */
int cmgpu_set_chr_order(cmgpu_ctx *ctx, const uint32_t *rank, uint32_t n_sequences);
/* --pairs-natural-chr-order (src/chromap.h:660-664, src/mapping_generator.cc:193-203): rank, over the sequences as the
 * records number them, that decides which end of a pair is written first; cmgpu_write_pairs_ranked orders the header by it. */
int cmgpu_set_pairs_chr_order(cmgpu_ctx *ctx, const uint32_t *rank, uint32_t n_sequences);
/* Before there is an index to make a context with: initialises the HIP runtime on the device, loads the library's device
 * code and maps 2 000 made-up pairs against a made-up 64 kb reference, from FASTQ text to BED text, in a context of its own
 * that is destroyed again -- hardware queues, scratch memory and sort plans a process otherwise pays for inside its first
 * batch (tens of milliseconds).  Optional; once per device and process; thread-safe; errors of the dry run are ignored. */
int cmgpu_warm_up(int device_id);

/* A further context over the SAME resident index and reference (no copy; the parent must outlive it).
 * Contexts are single-caller, so this is how one GPU keeps several batches in flight: one host
 * thread and one context per batch; their kernels share the compute units. */
int cmgpu_create_shared(const cmgpu_ctx *parent, cmgpu_ctx **out);
int cmgpu_destroy(cmgpu_ctx *ctx);
/* ctx may be NULL (returns the last error of a failed cmgpu_create*). */
const char *cmgpu_last_error(const cmgpu_ctx *ctx);
/* the message of the last failed call made BY THE CALLING THREAD (the per-file scans of a batch -- cmgpu_fastq_scan / _scan_bgzf -- may run
 * side by side on one ctx; cmgpu_last_error(ctx) then holds whichever failed last) */
const char *cmgpu_last_error_thread(void);

/* Replaces the taskloop body src/chromap.h:892-1143 for one batch: adapter trimming,
 * minimizers, index probe, candidate generation, mate rescue, pair filter, verification,
 * best-pair selection, coordinates and MAPQ.  `in` holds HOST pointers; records are
 * written to the caller's host buffer `out` (capacity in records; n_pairs *
 * max_num_best_mappings always suffices; a pair's records are adjacent, best-mapping index increasing).  Record order is unspecified (a total-order sort follows in the reference:
 * src/mapping_processor.h:117-159).  stats may be NULL; counters are ACCUMULATED.
 * A batch must start on a read_batch_size boundary of the input file for the reservoir
 * sampling of multi-mappers to reproduce the reference. */
/* out may be NULL (capacity 0): the records then stay resident for cmgpu_store_append_resident /
 * cmgpu_records_to_device and only their count is returned (same for the other cmgpu_map_* calls). */
int cmgpu_map_pairs(cmgpu_ctx *ctx, const cmgpu_batch *in, cmgpu_record *out, uint64_t out_capacity,
                    uint64_t *n_out, cmgpu_stats *stats);

/* One batch in flight: cmgpu_map_pairs_async returns at once and a worker thread of the library
 * uploads and maps the batch while the caller parses the next one (the reference overlaps its
 * "load next batch" task with the mapping taskloop the same way, src/chromap.h:871-877).
 * cmgpu_wait joins it; out may be NULL to leave the records resident.  Between the two calls the
 * ctx must not be used and the batch's buffers (and *stats) must stay valid. */
int cmgpu_map_pairs_async(cmgpu_ctx *ctx, const cmgpu_batch *in, cmgpu_stats *stats);
int cmgpu_wait(cmgpu_ctx *ctx, cmgpu_record *out, uint64_t out_capacity, uint64_t *n_out);

/* ---- the host-buffer boundary at the link's rate --------------------------------------------------------
 * Page-locked host memory for batch buffers and record arrays (cmgpu_host_alloc, or cmgpu_host_register on the caller's
 * own allocation), and a pipelined entry: cmgpu_submit_pairs starts the upload of the NEXT batch on a copy stream and
 * returns; cmgpu_map_submitted waits for that upload, maps the batch and downloads its records compacted (pair order
 * kept) -- so the upload of batch c+1 runs under the kernels of batch c, like the reference's load-next-batch task
 * beside its mapping taskloop (src/chromap.h:871-877):
 *     cmgpu_submit_pairs(ctx, &b[0]);
 *     for (c = 0; c < n; ++c) { if (c + 1 < n) cmgpu_submit_pairs(ctx, &b[c + 1]); cmgpu_map_submitted(ctx, out[c], cap, &k, &st); }
 * Up to two batches may be submitted and not yet mapped.  A submitted batch's buffers must stay valid until its
 * cmgpu_map_submitted returns; parking slots 6 and 7 of cmgpu_swap_resident_batch serve the uploads. */
void *cmgpu_host_alloc(uint64_t bytes);
void cmgpu_host_free(void *p);
int cmgpu_host_register(void *p, uint64_t bytes);
int cmgpu_host_unregister(void *p);
int cmgpu_submit_pairs(cmgpu_ctx *ctx, const cmgpu_batch *in);
int cmgpu_map_submitted(cmgpu_ctx *ctx, cmgpu_record *out, uint64_t out_capacity, uint64_t *n_out, cmgpu_stats *stats);
/* The same with the record download left running: cmgpu_map_submitted_async maps the oldest submitted batch, compacts its
 * records and queues their copy to `out` (page-locked: cmgpu_host_alloc / cmgpu_host_register) on a copy stream of its own, so
 * the copy runs under the NEXT batch's kernels -- the reference hands a finished batch's mappings to its output task the same
 * way while the next taskloop runs (src/chromap.h:871-877, mapping_writer.h:166-376).  cmgpu_records_wait returns when the
 * oldest pending download is complete and gives its record count; `out` must not be read before.  Up to two downloads may be
 * pending:
 *     cmgpu_submit_pairs(ctx, &b[0]);
 *     for (c = 0; c < n; ++c) {
 *       if (c + 1 < n) cmgpu_submit_pairs(ctx, &b[c + 1]);
 *       cmgpu_map_submitted_async(ctx, out[c & 1], cap, &st);
 *       if (c > 0) { cmgpu_records_wait(ctx, &k); consume(out[(c - 1) & 1], k); }
 *     }
 *     cmgpu_records_wait(ctx, &k); consume(out[(n - 1) & 1], k); */
int cmgpu_map_submitted_async(cmgpu_ctx *ctx, cmgpu_record *out, uint64_t out_capacity, cmgpu_stats *stats);
int cmgpu_records_wait(cmgpu_ctx *ctx, uint64_t *n_out);

/* Single-end reads: replaces the taskloop body of Chromap::MapSingleEndReads
 * (src/chromap.h:385-472) for bulk data; records are MappingWithoutBarcode's constructor
 * arguments (src/bed_mapping.h:67-83) stored in the cmgpu_record layout: alignment-length
 * fields 0, fragment = the read's alignment, direction 1 = + strand. */
typedef struct cmgpu_single_batch {
  uint32_t n_reads;
  uint32_t first_read_id;
  const char *bases;
  const uint32_t *offsets; /* n_reads + 1 */
} cmgpu_single_batch;
int cmgpu_map_single(cmgpu_ctx *ctx, const cmgpu_single_batch *in, cmgpu_record *out, uint64_t out_capacity,
                     uint64_t *n_out, cmgpu_stats *stats);
/* BED for single-end bulk records: sort (src/bed_mapping.h:90-95), duplicate removal on the
 * start position (:96-99), MAPQ filter, Tn5 shift (:104-110), line src/mapping_writer.cc:44-52 */
int64_t cmgpu_write_bed_se(const char *const *names, uint32_t n_sequences, const cmgpu_params *params,
                           cmgpu_record *records, uint64_t n_records, const char *out_path);

/* ---- single-cell barcodes (K6) --------------------------------------------------------
 * cmgpu_set_whitelist: Chromap::LoadBarcodeWhitelist (src/chromap.cc:388-490): keys =
 * GenerateSeedFromSequence of every whitelist line (cmgpu_load_whitelist_file produces them).
 * cmgpu_compute_barcode_abundance: Chromap::ComputeBarcodeAbundance (src/chromap.cc:492-548)
 * over ALL barcodes of the input (host pointers), batch structure and stop rule included;
 * fails with CMGPU_EINVAL when fewer than 5% of the first batch are whitelisted (the reference
 * exits there).  cmgpu_map_pairs_barcoded: the taskloop body with CorrectBarcodeAt in front
 * (src/chromap.h:896-909, src/chromap.cc:572-799). */
int cmgpu_load_whitelist_file(const char *path, uint32_t barcode_length, uint64_t **keys_out, uint32_t *n_out);
int cmgpu_set_whitelist(cmgpu_ctx *ctx, const uint64_t *keys, uint32_t n_keys, uint32_t barcode_length);
/* the whitelist with the abundances of the pre-pass, copied to another context (one context per GPU: the pre-pass
 * runs on one of them) */
int cmgpu_copy_whitelist(cmgpu_ctx *dst, cmgpu_ctx *src);
/* single-end reads with cell barcodes: MappingWithBarcode (src/bed_mapping.h:11-56), src/chromap.h:385-472 */
int cmgpu_map_single_barcoded(cmgpu_ctx *ctx, const cmgpu_single_batch *in, const cmgpu_barcode_batch *barcodes,
                              cmgpu_record_bc *out, uint64_t out_capacity, uint64_t *n_out, cmgpu_stats *stats);
/* enabled = 0: --skip-barcode-check (src/chromap.cc:523), the 5% test of the abundance pre-pass is not applied */
int cmgpu_set_barcode_check(cmgpu_ctx *ctx, int enabled);
int cmgpu_compute_barcode_abundance(cmgpu_ctx *ctx, const char *barcode_bases, const uint32_t *barcode_offsets,
                                    uint32_t n_barcodes, uint64_t *num_sample_barcodes);
int cmgpu_map_pairs_barcoded(cmgpu_ctx *ctx, const cmgpu_batch *in, const cmgpu_barcode_batch *barcodes,
                             cmgpu_record_bc *out, uint64_t out_capacity, uint64_t *n_out, cmgpu_stats *stats);
/* BED with the barcode column and cell-level duplicate removal (src/mapping_writer.cc:119-131,
 * src/bed_mapping.h:145-159; remove_pcr_duplicates_at_bulk_level == false as --preset atac sets). */
int64_t cmgpu_write_bed_pe_bc(const char *const *names, uint32_t n_sequences, const cmgpu_params *params,
                              cmgpu_record_bc *records, uint64_t n_records, uint32_t barcode_length,
                              const char *out_path);

/* Device-resident variant used for throughput measurement: inputs are uploaded once,
 * mapping runs on HBM-resident data and leaves the records in HBM. */
int cmgpu_upload_batch(cmgpu_ctx *ctx, const cmgpu_batch *in);
int cmgpu_map_resident(cmgpu_ctx *ctx, uint64_t *n_out, cmgpu_stats *stats);
int cmgpu_download_records(cmgpu_ctx *ctx, cmgpu_record *out, uint64_t out_capacity, uint64_t *n_out);
/* Size / content of the resident index (two-step: query sizes, then export).  buckets_out
 * receives 2*n_buckets uint64 ({key,val} per bucket, key == all ones marks an empty bucket),
 * occurrences_out n_occurrences uint64.  Used to give the CPU baseline the same index. */
int cmgpu_index_info(cmgpu_ctx *ctx, int32_t *kmer_size, int32_t *window_size, uint32_t *n_buckets,
                     uint32_t *n_occurrences, uint64_t *n_minimizers, uint64_t *n_keys);
int cmgpu_export_index(cmgpu_ctx *ctx, uint64_t *buckets_out, uint64_t *occurrences_out);

/* Dense copy of the resident batch's records into a caller-provided DEVICE buffer
 * (capacity in records) -- the send buffer of the multi-GPU record exchange. */
int cmgpu_records_to_device(cmgpu_ctx *ctx, void *device_dst, uint64_t capacity, uint64_t *n_out);
/* Same, grouped by the rank that owns the record's chromosome (cmgpu_exchange_owner_table):
 * counts[r] records for rank r, in rank order -- the send buffer and split sizes of an all-to-all. */
int cmgpu_records_partition(cmgpu_ctx *ctx, uint32_t world, void *device_dst, uint64_t capacity, uint64_t *counts);

/* ---- multi-GPU record exchange ----------------------------------------------
 * Read batches shard across GPUs with no collective on the mapping path; what the reference does
 * once per run on one host -- sort every chromosome's records and drop PCR duplicates
 * (MappingProcessor / MappingWriter::OutputTempMappings..., src/mapping_processor.h:100-202,
 * src/mapping_writer.h:166-376, fed by src/chromap.h:1305-1355) -- is done per chromosome OWNER:
 * after every batch each context sends its records to the rank that owns their chromosome (one
 * all-to-all, every record crosses xGMI once) and appends what it receives to its device-side record
 * store; cmgpu_store_format on every rank then yields that rank's section of the output, sections
 * concatenate in rank order (the output is chromosome-major).
 *   owner table   contiguous rid ranges (in the --chr-order rank space when one is set) such that the largest
 *                 owner's total sequence length is minimal: greedy in-order packing into bins of the smallest
 *                 size for which `world` bins suffice
 *   transport     RCCL, called by the library on the context's mapping stream (communicator made from a
 *                 ncclUniqueId the host distributes, or by cmgpu_exchange_init_all for the contexts of one
 *                 process), or two callbacks of the host's own communicator (MPI, a test harness).
 * cmgpu_exchange_step is collective: every rank calls it once per round, with an empty resident batch
 * when it has nothing to contribute. */
#define CMGPU_UNIQUE_ID_BYTES 128
typedef struct cmgpu_exchange_transport {
  void *user;
  /* mine[n] -> matrix[world * n], row r = rank r's `mine`.  Called twice per step: with n = world + 1 (records this
   * rank sends to each rank, then its record size) and, when world > 1, with n = 1 (a status word: a rank that cannot
   * take its share makes every rank leave the step before any payload moves) */
  int (*allgather_counts)(void *user, const uint64_t *mine, uint64_t *matrix, uint32_t n);
  /* send_dev: records grouped by destination rank (send_counts[world]); recv_dev: room for sum(recv_counts)
   * records, to be filled grouped by source rank; both are DEVICE pointers, record_bytes = 24 (32 with barcodes) */
  int (*alltoallv)(void *user, const void *send_dev, const uint64_t *send_counts, void *recv_dev,
                   const uint64_t *recv_counts, uint32_t world, uint32_t record_bytes);
} cmgpu_exchange_transport;
/* ncclGetUniqueId (call on one rank, hand the bytes to the others) */
int cmgpu_exchange_unique_id(void *id_out);
/* ncclCommInitRank on the context's device; collective over the `world` contexts */
int cmgpu_exchange_init(cmgpu_ctx *ctx, const void *unique_id, int rank, int world);
/* the contexts of ONE process, ctxs[i] becomes rank i (ncclCommInitAll over their devices) */
int cmgpu_exchange_init_all(cmgpu_ctx *const *ctxs, int n);
/* caller-provided transport instead of RCCL */
int cmgpu_exchange_init_external(cmgpu_ctx *ctx, const cmgpu_exchange_transport *t, int rank, int world);
/* owner rank of every sequence for `world` ranks (no exchange needs to be initialised) */
int cmgpu_exchange_owner_table(const cmgpu_ctx *ctx, uint32_t world, uint8_t *owner_out, uint32_t n_sequences);
/* partition the resident batch's records by owner -> exchange -> append the received records to this
 * context's store.  sent_per_rank: world entries or NULL. */
int cmgpu_exchange_step(cmgpu_ctx *ctx, uint64_t *sent_per_rank, uint64_t *n_received);
int cmgpu_exchange_info(const cmgpu_ctx *ctx, int *rank, int *world, uint64_t *records_sent, uint64_t *records_received);
/* The communication plan of one cmgpu_exchange_step round for `rank`, given the world x world count matrix (row r = the
 * records rank r sends to every rank) that the round's first all-gather hands to every rank: the collectives, the local copy
 * and the grouped sends / receives the step posts, in its order.  A pure host function (no device, no RCCL): multi-process
 * callers and tests replay it for all ranks to see that a round's posts meet (every send has its receive, every rank calls
 * the same collectives -- also a rank without records).  capacity < *n_ops: CMGPU_ECAPACITY (ops == NULL: just the count). */
typedef struct cmgpu_exchange_op {
  uint32_t kind;    /* CMGPU_EX_* */
  uint32_t peer;    /* send: destination, receive: source, copy: the rank itself */
  uint64_t records; /* records moved (all-gathers: 64-bit words contributed per rank) */
} cmgpu_exchange_op;
enum { CMGPU_EX_ALLGATHER_COUNTS = 0, CMGPU_EX_ALLGATHER_STATUS = 1, CMGPU_EX_COPY_SELF = 2, CMGPU_EX_SEND = 3, CMGPU_EX_RECV = 4 };
int cmgpu_exchange_plan(uint32_t rank, uint32_t world, const uint64_t *matrix, cmgpu_exchange_op *ops, uint32_t capacity, uint32_t *n_ops);
int cmgpu_exchange_finalize(cmgpu_ctx *ctx);
/* host <-> device copy through the library's HIP runtime, for a host-staged transport; kind 1: host -> device, 2: device -> host */
int cmgpu_memcpy(cmgpu_ctx *ctx, void *dst, const void *src, uint64_t bytes, int kind);

/* ---- --SAM --------------------------------------------------------------
 * With params.output_format == CMGPU_FORMAT_SAM the reported mappings are aligned with the
 * banded affine-gap DP the reference uses for SAM (ksw_semi_global3, src/ksw.cc:505-626, called
 * from src/mapping_generator.h:723-761, 807-854): start / end come from that alignment (MAPQ is
 * computed from them), and every reported read carries CIGAR, NM and MD
 * (GenerateNMAndMDTag, src/alignment.cc:85-139).  cmgpu_sam_record = the arguments of SAMMapping's
 * constructor (src/sam_mapping.h:151-190, src/mapping_generator.cc:43-57, 84-108) except the
 * strings the host already holds (name, sequence, quality).  Slots: 2*i / 2*i+1 for pair i
 * (read 1 / read 2), i for single-end read i; valid == 0: the read has no record.
 * CIGAR words (BAM encoding len<<4|op) and MD text sit in fixed-size slots of the pools. */
#define CMGPU_SAM_CIGAR_CAP 64
typedef struct cmgpu_sam_record {
  uint32_t read_id;
  uint32_t rid;
  uint32_t pos;    /* 0-based start on the reference */
  uint32_t mpos;
  int32_t mrid;    /* -1: no mate */
  int32_t tlen;
  uint32_t nm;
  uint16_t flag;
  uint16_t n_cigar;
  uint16_t md_len;
  uint8_t mapq;
  uint8_t strand;  /* 1 = + (SAMMapping::is_rev_ stores exactly this) */
  uint8_t is_unique;
  uint8_t valid;
  uint16_t length_after_trim; /* bases of the read that were mapped (adapter trimming) */
} cmgpu_sam_record;
/* slots and MD bytes per slot of the last mapped batch */
int cmgpu_sam_layout(const cmgpu_ctx *ctx, uint64_t *n_slots, uint32_t *md_cap);
/* copies records, n_slots * CMGPU_SAM_CIGAR_CAP cigar words and n_slots * md_cap MD bytes to the host */
int cmgpu_download_sam(cmgpu_ctx *ctx, cmgpu_sam_record *records, uint32_t *cigar_pool, char *md_pool);
/* SAM text (src/mapping_writer.cc:312-356): @SQ header unless append, records sorted by
 * SAMMapping::operator< (src/sam_mapping.h:193-199), duplicate removal on operator== in the
 * low-memory or in-memory flavour, MAPQ filter.  names / bases / quals / offsets: the batch(es) the
 * slots refer to (mate-2 arrays NULL for single-end data). */
int64_t cmgpu_write_sam(const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const cmgpu_params *params,
                        const cmgpu_sam_record *records, uint64_t n_slots, int paired, const uint32_t *cigar_pool,
                        const char *md_pool, uint32_t md_cap, const char *const *names1, const char *const *names2,
                        const char *bases1, const char *quals1, const uint32_t *offsets1, const char *bases2,
                        const char *quals2, const uint32_t *offsets2, const char *out_path);
/* single-cell data: the (corrected) barcode keys of the batch last mapped with cmgpu_map_pairs_barcoded /
 * cmgpu_map_single_barcoded, one per pair / read (what the reference keeps in SAMMapping::cell_barcode_) */
int cmgpu_download_barcode_keys(cmgpu_ctx *ctx, uint64_t *keys);
/* cmgpu_write_sam for single-cell data: cell_barcode_ takes part in operator< / operator==
 * (src/sam_mapping.h:201-212) and every line ends with CB:Z:<barcode> (src/mapping_writer.cc:350-354).
 * barcode_keys: one per pair / read, in slot order */
int64_t cmgpu_write_sam_barcoded(const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const cmgpu_params *params,
                                 const cmgpu_sam_record *records, uint64_t n_slots, int paired, const uint32_t *cigar_pool,
                                 const char *md_pool, uint32_t md_cap, const char *const *names1, const char *const *names2,
                                 const char *bases1, const char *quals1, const uint32_t *offsets1, const char *bases2,
                                 const char *quals2, const uint32_t *offsets2, const uint64_t *barcode_keys, uint32_t barcode_length,
                                 const char *out_path);
/* the same with --barcode-translate (src/barcode_translator.h:43-101, src/mapping_writer.cc:350-354): the CB:Z: value goes through the
 * translation table, whose (inflated) text the caller hands over -- lines "to<TAB or ,>from".  A barcode that is not in the
 * table: CMGPU_EFORMAT (the reference exits with "Barcode does not exist in the translation table."). */
int64_t cmgpu_write_sam_barcoded_translated(const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const cmgpu_params *params,
                                            const cmgpu_sam_record *records, uint64_t n_slots, int paired, const uint32_t *cigar_pool,
                                            const char *md_pool, uint32_t md_cap, const char *const *names1, const char *const *names2,
                                            const char *bases1, const char *quals1, const uint32_t *offsets1, const char *bases2,
                                            const char *quals2, const uint32_t *offsets2, const uint64_t *barcode_keys, uint32_t barcode_length,
                                            const char *translate_table, uint64_t translate_table_bytes, const char *out_path);

/* ---- SAM output on the device -------------------------------------------------------------
 * Replaces the host writers above for runs that go through the device ingest: the SAMMapping objects the reference keeps per
 * mapped read (src/sam_mapping.h:151-212) stay in HBM, and MappingWriter<SAMMapping>::AppendMapping's text
 * (src/mapping_writer.cc:312-356) is rendered there from the read store (cmgpu_fastq_keep_reads).
 *   cmgpu_sam_store_append_resident  after a cmgpu_map_resident of a CMGPU_FORMAT_SAM context: the batch's valid slots -- record,
 *                                    mate, CIGAR words, MD bytes and, for barcoded batches, the pair's barcode key -- join a run-wide
 *                                    store, compacted (the fixed CIGAR / MD slots stay per batch); n_total = records in the store
 *   cmgpu_store_format_sam           sorts the store by SAMMapping::operator< (rid, pos, barcode, mrid, mpos, flag & 64, mapq,
 *                                    read_id), removes duplicates on operator== (low_memory_mode: the first record with the run's
 *                                    largest MAPQ; otherwise the last of the run), applies the MAPQ filter and renders one line per
 *                                    record into the context's text store: cmgpu_store_text / cmgpu_store_write_text /
 *                                    cmgpu_store_info then work as for BED and pairs.  The bytes equal cmgpu_write_sam* without
 *                                    the header; offsets are 64-bit (the text of a realistic run passes 4 GiB)
 *   cmgpu_write_sam_header           the @SQ lines, on the host; the text follows with cmgpu_store_write_text(path, 1) */
int cmgpu_sam_store_append_resident(cmgpu_ctx *ctx, uint64_t *n_total);
int cmgpu_sam_store_clear(cmgpu_ctx *ctx);
/* n_bytes: HBM the stored records take (records, offsets, CIGAR + MD, barcode keys) */
int cmgpu_sam_store_info(const cmgpu_ctx *ctx, uint64_t *n_records, uint64_t *n_bytes);
int cmgpu_store_format_sam(cmgpu_ctx *ctx, const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences,
                           const cmgpu_params *params, uint32_t barcode_length, uint64_t *n_lines, uint64_t *n_bytes);
int cmgpu_write_sam_header(const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const char *out_path);

/* ---- BAM output on the device (cm_bam.h) ------------------------------------------------------
 * The same SAM record store and read store, the same sort and the same selection (duplicates, MAPQ filter, --summary credit, the
 * checks for foreign records and translation misses) as cmgpu_store_format_sam; the selected records are rendered as BAM alignment
 * records (SAM spec 4.2: block_size, the 32 fixed bytes, read name, CIGAR words, 4-bit SEQ, QUAL, the tags NM (C / S / I by value),
 * MD:Z and -- for barcoded stores -- CB:Z) instead of lines.
 *   cmgpu_store_format_bam   leaves the records back to back, uncompressed, in the context's text store; *n_records counts them
 *                            (cmgpu_store_info's text_lines).  cmgpu_store_text / cmgpu_store_write_text fetch the bytes;
 *                            cmgpu_store_compress_text + cmgpu_bgzf_write make them the body of a BAM file (a record may straddle
 *                            two blocks: the format allows it).  A selected record whose read name has 255 bytes or more does not
 *                            fit l_read_name: CMGPU_EFORMAT, no output.  cmgpu_bgzf_index_tabix refuses a store made of BAM records.
 *                            The .bai index: cmgpu_bgzf_index_bai below (.csi: cmgpu_bgzf_index_csi_bam); bin is the spec's reg2bin(pos, pos + reference
 *                            length of the CIGAR).
 *   cmgpu_write_bam_header   the uncompressed header, on the host: "BAM\1", l_text and cmgpu_write_sam_header's @SQ lines, n_ref,
 *                            and per sequence l_name (with the NUL), the name, l_ref.  As BGZF blocks (cmgpu_bgzf_write_host_text)
 *                            in front of the compressed records and with cmgpu_bgzf_write_eof behind them it completes the file */
int cmgpu_store_format_bam(cmgpu_ctx *ctx, const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences,
                           const cmgpu_params *params, uint32_t barcode_length, uint64_t *n_records, uint64_t *n_bytes);
int cmgpu_write_bam_header(const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const char *out_path);

/* ---- --barcode-translate on the device (src/barcode_translator.h:42-101) -----------------------
 * A translation table per context, held in HBM: with one set, cmgpu_store_format writes column 4 of CMGPU_TEXT_BED_PE_BC /
 * CMGPU_TEXT_BED_SE_BC, and cmgpu_store_format_sam the CB:Z: value, as the table's names instead of ACGT (TagAlign and pairs
 * print no barcode; every other kind gives the bytes it gives without a table).  n_bytes and n_lines are the translated text's.
 *   table_text   the inflated text of the file (the caller does the gzopen): lines "to<TAB or ,>from".  The key is the 2-bit
 *                packing of `from` (other letters count as A); the last line of a repeated key wins; the LAST line's `from`
 *                length is the segment length; a line without a separator is skipped; `to` may be empty.  No usable line:
 *                CMGPU_EINVAL.  NULL / 0 clears the table.
 *   segments     a barcode of L bases is translated as L / from_length segments joined by '-', cut with the reference's shifts
 *                seed_i = ((key << (2 * i * from)) >> (2 * (n - 1) * from)) & mask on 64-bit values (:80-83) -- also where L is
 *                no multiple of from_length.  from_length > L: the column is empty.
 *   a miss       a line that would be printed (after duplicate removal, the MAPQ filter and the sequence check) whose barcode
 *                has a segment the table lacks: the format call returns CMGPU_EFORMAT, cmgpu_last_error is the reference's
 *                "Barcode does not exist in the translation table." and no text is published (cmgpu_store_info: 0 bytes).
 *   HBM          16 bytes per bucket, a power of two of buckets >= 2 x entries (>= 16), + the bytes of the `to` names.
 * cmgpu_copy_barcode_translation: the table of another context (one context per GPU, like cmgpu_copy_whitelist); a source
 * without a table clears the destination's. */
int cmgpu_set_barcode_translation(cmgpu_ctx *ctx, const char *table_text, uint64_t n_bytes);
int cmgpu_barcode_translation_info(const cmgpu_ctx *ctx, uint32_t *n_entries, uint32_t *from_length, uint64_t *n_bytes_hbm);
int cmgpu_copy_barcode_translation(cmgpu_ctx *dst, cmgpu_ctx *src);
/* The image cmgpu_set_barcode_translation uploads, made without a device (a pure host function):
 *   buckets   2 x uint64 each, {key, to_offset << 32 | to_length}; a VALUE word of all ones marks an empty bucket (all ones is a
 *             legal key: 32 T's).  *n_buckets is a power of two >= 2 x entries (>= 16).  A key is in the first free bucket from
 *             ((key * 0x9E3779B97F4A7C15) >> 32) & (n_buckets - 1) onwards, wrapping at the table's end; keys are inserted in
 *             increasing order.
 *   blob      the `to` names back to back (no terminators), *blob_bytes of them
 * buckets == NULL (or blob == NULL with names to store): sizes only.  bucket_capacity (in buckets) or blob_capacity too small:
 * CMGPU_ECAPACITY with the sizes reported.  No usable line: CMGPU_EINVAL. */
int cmgpu_barcode_translation_pack(const char *table_text, uint64_t n_bytes, uint64_t *buckets, uint64_t bucket_capacity, char *blob,
                                   uint64_t blob_capacity, uint64_t *n_buckets, uint64_t *blob_bytes, uint32_t *from_length);
/* One barcode key through a packed image on the host, with the lookup, segment and render functions the device writers use:
 * out receives the translated column (*n_out bytes, no terminator).  A segment the table lacks: CMGPU_EFORMAT; capacity < *n_out:
 * CMGPU_ECAPACITY with *n_out set. */
int cmgpu_barcode_translate_host(const uint64_t *buckets, uint64_t n_buckets, const char *blob, uint32_t from_length, uint64_t barcode_key,
                                 uint32_t barcode_length, char *out, uint64_t capacity, uint64_t *n_out);

/* ---- device-side post-processing -------------------------------------
 * Replaces, for BED output: MappingProcessor::SortOutputMappings / RemovePCRDuplicate
 * (src/mapping_processor.h:100-202), the low-memory merge's duplicate handling
 * (src/mapping_writer.h:166-376), ApplyTn5ShiftOnMappings, the MAPQ filter and
 * MappingWriter::AppendMapping (src/mapping_writer.cc:44-52, 72-83, 119-131).
 * Batches append their records to a store in HBM; one call sorts (radix sort on the
 * operator< key), removes duplicates (low_memory_mode: first record with the maximal MAPQ of an
 * operator== run; otherwise RemovePCRDuplicate's last record of the run, Tn5 shift applied
 * before the sort as src/chromap.h:1323-1331 does), filters, and renders the text in HBM.
 * The bytes equal cmgpu_write_bed_* / the reference's output file. */
#define CMGPU_TEXT_BED_PE 0
#define CMGPU_TEXT_BED_SE 1
#define CMGPU_TEXT_BED_PE_BC 2
#define CMGPU_TEXT_TAGALIGN_PE 3    /* --TagAlign, paired-end bulk: two lines per fragment (src/mapping_writer.cc:84-117) */
#define CMGPU_TEXT_TAGALIGN_PE_BC 4
#define CMGPU_TEXT_BED_SE_BC 5      /* single-end single-cell BED: MappingWithBarcode (src/bed_mapping.h:11-56, src/mapping_writer.cc:6-25) */
#define CMGPU_TEXT_TAGALIGN_SE_BC 6 /* --TagAlign, single-end single-cell: chr start end N mapq strand (src/mapping_writer.cc:26-34) */
int cmgpu_store_clear(cmgpu_ctx *ctx);
/* room for n_records ahead of time (the store otherwise doubles on demand: allocation + copy + synchronous free) */
int cmgpu_store_reserve(cmgpu_ctx *ctx, uint64_t n_records, int barcoded);
/* appends the records of the last cmgpu_map_* call (still resident); n_total = store size.  The store keeps the kind of its first append -- bulk or
   barcoded, cmgpu_pairs_record or cmgpu_record -- until cmgpu_store_clear: an append of another kind is CMGPU_EINVAL, and cmgpu_store_format_pairs*
   judges the store by that kind whatever batch the context mapped last */
int cmgpu_store_append_resident(cmgpu_ctx *ctx, uint64_t *n_total);
/* appends n records from a host or device array; barcoded = 0: cmgpu_record entries,
 * barcoded = 1: cmgpu_record_bc entries -- e.g. the receive buffer of the multi-GPU exchange */
int cmgpu_store_append(cmgpu_ctx *ctx, const void *records, uint64_t n, int on_device, int barcoded);
int cmgpu_store_format(cmgpu_ctx *ctx, int kind, const char *const *names, uint32_t n_sequences, const cmgpu_params *params,
                       uint32_t barcode_length, uint64_t *n_lines, uint64_t *n_bytes);
/* --preset hic: the store holds cmgpu_pairs_record entries (cmgpu_store_append_resident after a paired-end split-alignment batch);
 * sorted as MappingWriter<PairsMapping> sorts them (src/pairs_mapping.h:41-47), MAPQ filter, one text line per record
 * (src/mapping_writer.cc:400-423).  read_names: the names of reads read_id_base .. read_id_base + n_read_names - 1
 * concatenated, read_name_offsets[n_read_names + 1] into it.  The header lines: cmgpu_write_pairs_header.
 * The bytes equal cmgpu_write_pairs' lines. */
int cmgpu_store_format_pairs(cmgpu_ctx *ctx, const char *const *names, uint32_t n_sequences, const cmgpu_params *params,
                             const char *read_names, const uint64_t *read_name_offsets, uint32_t n_read_names, uint32_t read_id_base,
                             uint64_t *n_lines, uint64_t *n_bytes);
/* cmgpu_store_format_pairs with the read names taken from the context's name store (cmgpu_fastq_keep_names) instead of a host
 * blob: MappingWriter<PairsMapping>::AppendMapping's read_name column (src/mapping_writer.cc:400-423) comes from HBM, where the
 * device ingest left it -- no upload, no copy.  Same order, filter and bytes. */
int cmgpu_store_format_pairs_resident(cmgpu_ctx *ctx, const char *const *names, uint32_t n_sequences, const cmgpu_params *params,
                                      uint64_t *n_lines, uint64_t *n_bytes);
int cmgpu_write_pairs_header(const char *const *names, const uint32_t *lengths, uint32_t n_sequences, const uint32_t *pairs_rank,
                             const char *out_path);
int cmgpu_store_text(cmgpu_ctx *ctx, char *out, uint64_t capacity);
int cmgpu_store_write_text(cmgpu_ctx *ctx, const char *path, int append);
int cmgpu_store_info(const cmgpu_ctx *ctx, uint64_t *n_records, uint64_t *text_bytes, uint64_t *text_lines);
/* ---- BGZF output compressed on the device (cm_deflate.h, cm_bgzf_out.hip) -------------------
 * The reference writes plain text and leaves the compression to bgzip; here the rendered text becomes BGZF blocks (SAM spec 4.1) in
 * HBM: block i holds the text bytes [i * 0xff00, (i + 1) * 0xff00) as one dynamic-Huffman DEFLATE block, or a stored one where that
 * would not be smaller.  The blocks are a function of the text alone.  They land in the context's compressed store, which the next
 * compression replaces.
 *   cmgpu_bgzf_compress         n_bytes at `text` (on_device != 0: a device pointer); n_bytes == 0: no block
 *   cmgpu_store_compress_text   the text store left by cmgpu_store_format*; the text store stays as it is
 *   cmgpu_bgzf_info             blocks and bytes of the compressed store, and the text bytes they hold
 *   cmgpu_bgzf_download         the blocks to the host (capacity >= the store's bytes, else CMGPU_ECAPACITY)
 *   cmgpu_bgzf_write            the blocks to a file (append != 0: behind what it holds), WITHOUT the end-of-file block: the
 *                               sections of several contexts, or header lines and a context's text, follow each other in one file
 *   cmgpu_bgzf_write_host_text  n bytes of host text (the @SQ lines, the pairs header) as stored BGZF blocks built on the host
 *   cmgpu_bgzf_write_eof        appends the 28-byte empty block that ends a BGZF file: once, last */
int cmgpu_bgzf_compress(cmgpu_ctx *ctx, const void *text, uint64_t n_bytes, int on_device, uint64_t *n_blocks, uint64_t *n_out);
int cmgpu_store_compress_text(cmgpu_ctx *ctx, uint64_t *n_blocks, uint64_t *n_out);
int cmgpu_bgzf_info(const cmgpu_ctx *ctx, uint64_t *n_blocks, uint64_t *n_bytes, uint64_t *n_text_bytes);
int cmgpu_bgzf_download(cmgpu_ctx *ctx, void *out, uint64_t capacity);
int cmgpu_bgzf_write(cmgpu_ctx *ctx, const char *path, int append);
int cmgpu_bgzf_write_host_text(const char *path, const void *text, uint64_t n, int append);
int cmgpu_bgzf_write_eof(const char *path);
/* ---- tabix index of the compressed store, built on the device (cm_tabix.h, cm_tabix.hip) -------
 * The .tbi a BGZF BED / TagAlign file needs (SAM/tabix spec, preset `bed`: sequence column 1, begin 2, end 3, 0-based half-open,
 * comment character '#'), made from what is in HBM once the compressor is done: the text it compressed, and the blocks' sizes.
 * The text must be sorted as the BED writers sort it: every name in one run of lines, starts ascending within a run; it is empty
 * or ends with a newline; columns 2 and 3 are decimal; no end beyond 2^29 (the format's limit).  A text that is not -- paired
 * TagAlign, pairs, SAM -- is refused with CMGPU_EFORMAT and a message that names the first offending line; the context stays usable.
 * Bins are written in ascending number, a bin's chunks in file order, adjacent chunks joined where the second begins in the block
 * in which the first ends (htslib's rule); every reference ends with the pseudo-bin 37450; the linear index is back-filled.
 *   cmgpu_bgzf_index_tabix  indexes the text of the last cmgpu_bgzf_compress / cmgpu_store_compress_text against its blocks, which
 *                           will stand at base_offset in the file (the bytes written before them: header blocks).  The payload
 *                           (the uncompressed .tbi) stays with the context; *n_bytes its size.  CMGPU_EINVAL: nothing compressed
 *                           yet, or the text store has been rendered anew since
 *   cmgpu_tabix_download    the payload (capacity >= its size, else CMGPU_ECAPACITY)
 *   cmgpu_tabix_write       the payload as a BGZF file: stored blocks written by the host, then the end-of-file block */
int cmgpu_bgzf_index_tabix(cmgpu_ctx *ctx, uint64_t base_offset, uint64_t *n_bytes);
int cmgpu_tabix_download(cmgpu_ctx *ctx, void *out, uint64_t capacity);
int cmgpu_tabix_write(cmgpu_ctx *ctx, const char *path);
/* ---- BAM index of the compressed store, built on the device (cm_bai.h, cm_tabix.hip) -----------
 * The .bai a coordinate-sorted BAM file needs (SAM spec 5.2), made from what is in HBM once the compressor is done: the records it
 * compressed, where each of them starts, and the blocks' sizes.  The binning scheme, the 16 kb linear index, the chunk rules and the
 * pseudo-bin 37450 are the tabix index's, and so are the kernels from the raw chunks on; the keys are fields of the binary records
 * (refID, pos, the CIGAR's reference length, flag bit 4).  The records must be a chain -- each ends where the next one starts -- sorted
 * by (refID, pos), every refID in 0 .. n_ref - 1 (no unmapped records: n_no_coor is 0), no end beyond 2^29 (the format's limit;
 * `samtools index -c` builds a .csi for such a file).  Anything else is refused with CMGPU_EFORMAT and a message that names the first
 * offending record and the cause; the context stays usable.  A reference without records has no bin, no pseudo-bin and no window.
 * Sparse bins are not folded into their parents as htslib does: the index is valid and differs from `samtools index`'s bytes.
 *   cmgpu_bam_keep_starts   on != 0: from now on cmgpu_store_format_bam keeps the offsets of the records it writes (8 bytes each, in
 *                           HBM).  They belong to that rendering: the next cmgpu_store_format* or cmgpu_store_clear drops them.
 *                           Off by default; a context that never turns it on runs what it ran before
 *   cmgpu_bgzf_index_bai    indexes the records of the last cmgpu_bgzf_compress / cmgpu_store_compress_text against its blocks, which
 *                           will stand at base_offset in the file (the bytes written before them: the header's blocks).  n_ref: the
 *                           header's.  starts == NULL: the kept starts of the text store (CMGPU_EINVAL with a message where none
 *                           were kept or the store does not hold BAM records); else a host array of n_records + 1 offsets, the last
 *                           one the number of bytes, for records the caller compressed itself.  The payload (the .bai file's bytes)
 *                           stays with the context; *n_bytes its size.  CMGPU_EINVAL also: nothing compressed yet, or the text
 *                           store has been rendered anew since
 *   cmgpu_bai_download      the payload (capacity >= its size, else CMGPU_ECAPACITY)
 *   cmgpu_bai_write         the payload as a file (a .bai is not compressed); on failure the file is removed */
int cmgpu_bam_keep_starts(cmgpu_ctx *ctx, int on);
int cmgpu_bgzf_index_bai(cmgpu_ctx *ctx, uint64_t base_offset, uint32_t n_ref, const uint64_t *starts, uint64_t n_records, uint64_t *n_bytes);
int cmgpu_bai_download(cmgpu_ctx *ctx, void *out, uint64_t capacity);
int cmgpu_bai_write(cmgpu_ctx *ctx, const char *path);
/* ---- CSI index of the compressed store, built on the device (cm_tabix.h, cm_bai.h, cm_tabix.hip) --
 * The .csi (SAM spec 5.3, CSIv1) of the same stores: the .tbi's and the .bai's stages with the number of levels as a parameter.
 * min_shift is 14; depth is 1 .. 6 (else CMGPU_EINVAL) and an end may reach 2^(14 + 3 * depth) -- 2^29 at depth 5, as the .tbi and
 * .bai; positions are 32-bit, so depth 6 takes ends up to 0xffffffff, not 2^32.  There is no linear index: every bin carries
 * loffset, the back-filled 16 kb window value at the bin's first position (htslib's rule), computed on the device; the pseudo-bin
 * ((1 << (3 * depth + 3)) - 1) / 7 + 1 has loffset 0.  Bins are not folded.  What is refused, and with which words, is what the .tbi
 * / .bai calls refuse; the RANGE message names the limit of the depth in use.
 *   cmgpu_bgzf_index_csi_bam    the BAM flavour (l_aux = 0) of the records cmgpu_bgzf_index_bai would index; the same arguments
 *                               (starts == NULL: the kept starts) and depth
 *   cmgpu_bgzf_index_csi_tabix  the tabix flavour (what `tabix -C -p bed` writes: aux holds the tabix header's format, columns, meta,
 *                               skip and names) of the text cmgpu_bgzf_index_tabix would index
 *   cmgpu_csi_download          the last payload of either (capacity >= its size, else CMGPU_ECAPACITY); CMGPU_EINVAL: none built
 *   cmgpu_csi_write             the payload as a BGZF file, as cmgpu_tabix_write writes a .tbi; CMGPU_EINVAL: none built */
int cmgpu_bgzf_index_csi_bam(cmgpu_ctx *ctx, uint64_t base_offset, uint32_t n_ref, const uint64_t *starts, uint64_t n_records, uint32_t depth, uint64_t *n_bytes);
int cmgpu_bgzf_index_csi_tabix(cmgpu_ctx *ctx, uint64_t base_offset, uint32_t depth, uint64_t *n_bytes);
int cmgpu_csi_download(cmgpu_ctx *ctx, void *out, uint64_t capacity);
int cmgpu_csi_write(cmgpu_ctx *ctx, const char *path);
/* --allocate-multi-mappings (MappingProcessor::AllocateMultiMappings, src/mapping_processor.h:319-440): with
 * params->allocate_multi_mappings and without low_memory_mode, cmgpu_store_format gives every read whose surviving records have
 * MAPQ < 4 to one of them, drawn with probability proportional to the uni-mappings (MAPQ >= 4) within
 * multi_mapping_allocation_distance of it, and drops the reads that have none; then the MAPQ filter and the text as usual.  The
 * counts of the last cmgpu_store_format, the reference's "Got all N multi-mappings", "Allocated K multi-mappings" and "# multi-mappings
 * that have no uni-mapping overlaps: M"; zeros when no allocation ran.  Not with --summary counting, nor on a store filled by the
 * multi-GPU exchange (CMGPU_EINVAL); cmgpu_store_format_pairs* and cmgpu_store_format_sam refuse the flag. */
int cmgpu_store_allocation_info(const cmgpu_ctx *ctx, uint64_t *n_multi, uint64_t *n_allocated, uint64_t *n_without_overlap);

/* ---- FASTQ ingest on the device ---------------------------------------
 * Replaces, for 4-line FASTQ text, kseq_read + SequenceBatch::LoadOneSequenceAndSaveAt
 * (src/sequence_batch.cc:22-62): the host hands over raw (inflated) file bytes chunk by chunk;
 * lines, records, the skip of empty sequences and the SoA batch are built in HBM.
 * stream: 0 = read 1, 1 = read 2, 2 = cell barcodes (bases + qualities).
 *   cmgpu_fastq_scan   uploads one chunk (< 4 GiB) and counts its complete, non-empty records;
 *                      final_chunk != 0: the text ends the file (a missing last newline is fine).
 *                      CMGPU_EFORMAT: not 4-line FASTQ (other layouts: cmgpu_fastq_set_layout, CMGPU_FASTX_FREE).
 *                      Scans (this call and cmgpu_fastq_scan_bgzf) of DIFFERENT streams of one context may be
 *                      made from different host threads at the same time: each stream has a HIP stream and
 *                      scratch of its own; every other call on a context is one thread at a time.
 *   cmgpu_fastq_take   gathers the first n of them as this stream's part of the NEXT batch (staging buffers) and
 *                      returns how many bytes of the chunk they (and skipped records) cover --
 *                      the host resubmits the rest in front of the next chunk.
 *   cmgpu_fastq_commit declares the batch (n records taken from every participating stream): the staging buffers
 *                      become the resident batch; cmgpu_map_resident then maps it.
 * Overlap: scans and takes touch only the streams' own buffers, HIP streams and the staging buffers, so ONE thread may
 * scan and take the next batch while ANOTHER is inside cmgpu_map_resident / cmgpu_store_append_resident with the
 * committed one (chromap-amd does; tests/test_gpu_ingest.py::test_next_batch_taken_while_the_last_is_mapped).
 * cmgpu_fastq_commit itself must not run beside a mapping call of the same context.
 * Read names: cmgpu_fastq_keep_names makes a stream's takes gather the records' names as well (staging, like the bases); the
 * commit appends them to a run-wide name store in HBM (cmgpu_names_info / cmgpu_download_names / cmgpu_names_clear), from which
 * cmgpu_store_format_pairs_resident renders the pairs text -- so --preset hic / --pairs runs use this ingest too. */
/* --read-format for one stream (SequenceEffectiveRange, src/sequence_effective_range.h, src/chromap.cc:825-866):
 * up to four [start, end] base ranges (0-based, inclusive, end -1 = last base) are concatenated, then the result is
 * reverse-complemented (bases) / reversed (qualities) when strand is '-'.  Applies to the following cmgpu_fastq_take calls. */
int cmgpu_fastq_set_format(cmgpu_ctx *ctx, int stream, int n_ranges, const int32_t *starts, const int32_t *ends, char strand);
int cmgpu_fastq_scan(cmgpu_ctx *ctx, int stream, const char *text, uint64_t n_bytes, int final_chunk, uint32_t *n_records);
/* BGZF input (bgzip: gzip members of at most 64 KiB with their size in a 'BC' extra field) inflated ON THE DEVICE: `blocks` holds
 * whole COMPRESSED blocks as they stand in the file (the end-of-file marker block may be among them); a lane per block decodes
 * its DEFLATE codes, a wave per block copies the matches inside the block's place in the stream's text and checks its CRC-32 --
 * what zlib's gzread does for the reference, one stream per file (src/sequence_batch.cc:22-62).  The text stays on the device: what cmgpu_fastq_take does not
 * consume is kept in front of the blocks of the next call (the host does not resubmit anything; a call after which nothing is
 * taken simply extends the text).  CMGPU_EFORMAT: not BGZF, a truncated or a damaged block (cmgpu_last_error says which), or not
 * 4-line FASTQ.  A call of cmgpu_fastq_scan on the stream returns it to host-resubmitted text. */
int cmgpu_fastq_scan_bgzf(cmgpu_ctx *ctx, int stream, const void *blocks, uint64_t n_bytes, int final_chunk, uint32_t *n_records);
int cmgpu_fastq_take(cmgpu_ctx *ctx, int stream, uint32_t n, uint64_t *bytes_consumed);
/* Record layout of a stream (0 = read 1, 1 = read 2, 2 = barcodes); applies to the following cmgpu_fastq_scan / _scan_bgzf calls.
 * CMGPU_FASTX_STRICT4 (default): four lines per record, as described above, with its messages.
 * CMGPU_FASTX_FREE: what kseq_read reads (src/kseq.h:177-218) -- sequence and quality wrapped over any number of lines, FASTA records,
 * blank lines between records, CRLF, no final newline.  Over the lines of the text (split at '\n') kseq is this automaton on a line's
 * first byte: SEEK skips lines up to one that starts with '@' or '>' (kseq.h:183), the header, whose name ends at the first isspace() byte
 * (kseq.h:188).  SEQUENCE: a '+' line starts the quality; an '@' / '>' line ends the record without quality and is the next header
 * (kseq.h:194-199); empty lines are skipped; other lines are appended without their '\r' (kseq.h:141); the end of the final chunk ends the
 * record.  QUALITY: the rest of the '+' line is ignored (kseq.h:211); lines -- at least one, whatever their first byte -- are appended
 * until the quality is as long as the sequence (kseq.h:213); another length, or the end of the text first, is kseq's -2 (kseq.h:212,216):
 * CMGPU_EFORMAT "truncated quality", for every stream.  Records with an empty sequence give no record and no name
 * (src/sequence_batch.cc:27-30).  Refused with CMGPU_EFORMAT, never read differently from kseq: a skipped line in SEEK state that is
 * not blank; a line holding only '\r' where the sequence or the quality is still empty (kseq keeps that '\r'); a record without quality
 * on a stream that needs qualities (cmgpu_fastq_keep_reads, the barcode stream -- the reference cannot write SAM for FASTA reads either);
 * records with quality and records without in one stream (kseq reads such a mix, and with it half a record behind a FASTQ file's last
 * whole one; a file of either kind alone is read, whatever its markers); lines or sequences of 256 MiB and more.  Records do not depend on how the text is cut into chunks: a non-final scan counts a record
 * only when the chunk proves it complete (FASTQ: the quality reached the sequence's length; FASTA: the next header line is whole), and
 * cmgpu_fastq_take's bytes_consumed ends behind the last taken record as before.
 * The scan tries the four-line path first: text that passes it costs what it costs in CMGPU_FASTX_STRICT4, except that the quality's
 * length is checked for every stream.  Only a chunk that fails it is resolved by the general path (cm_fastx.h), on the same resident
 * text and line index.  cmgpu_fastq_scan_info: whether the stream's last scan took the general path, and the chunk's number of lines.
 * An unknown layout, or a change while inflated text of the stream is kept on the device (BGZF mode), is CMGPU_EINVAL. */
#define CMGPU_FASTX_STRICT4 0
#define CMGPU_FASTX_FREE 1
int cmgpu_fastq_set_layout(cmgpu_ctx *ctx, int stream, int layout);
int cmgpu_fastq_scan_info(const cmgpu_ctx *ctx, int stream, int *general_path, uint32_t *n_lines);
int cmgpu_fastq_commit(cmgpu_ctx *ctx, uint32_t n, uint32_t first_read_id, int paired, int barcoded);
/* Replaces kseq's name.s (ks_getuntil(ks, 0, &seq->name, &c), kseq.h:188, kept per read by SequenceBatch::LoadOneSequenceAndSaveAt,
 * src/sequence_batch.cc:36) for the device ingest: with on != 0 every following cmgpu_fastq_take of the stream (0 = read 1 or
 * 1 = read 2; one of them per context) also gathers, for the records it takes, the bytes of the header line after the '@' up to, not
 * including, the first isspace() byte -- the comment is dropped, an empty name has length 0, records with an empty sequence have no
 * name as they have no record; --read-format does not touch names.  cmgpu_fastq_commit then appends the batch's names to the
 * context's name store, indexed by read_id - read_id_base: batches must be committed with consecutive read ids (a gap:
 * CMGPU_EINVAL, nothing is committed); no room in HBM: CMGPU_ENOMEM.  Call it before the first scan of a run; on = 0 (the default)
 * costs nothing. */
int cmgpu_fastq_keep_names(cmgpu_ctx *ctx, int stream, int on);
/* empties the name store (a new run; the next commit sets read_id_base) */
int cmgpu_names_clear(cmgpu_ctx *ctx);
int cmgpu_names_info(const cmgpu_ctx *ctx, uint64_t *n_names, uint64_t *n_bytes, uint32_t *read_id_base);
/* the name store on the host: the names back to back in blob (capacity >= n_bytes), offsets[n_names + 1] into it -- what the host
 * parser keeps in SequenceBatch::GetSequenceNameAt (src/sequence_batch.h); for tests and host-side writers */
int cmgpu_download_names(cmgpu_ctx *ctx, char *blob, uint64_t blob_capacity, uint64_t *offsets);
/* Whole reads for SAM output.  Replaces what SequenceBatch::LoadOneSequenceAndSaveAt keeps of every record (src/sequence_batch.cc:22-62:
 * name, sequence, quality) for the device ingest: with on != 0 every following cmgpu_fastq_take of read 1 (and, for paired batches,
 * read 2) also gathers the taken records' names (kseq's rule, as cmgpu_fastq_keep_names) and quality lines -- at the bases' offsets,
 * --read-format applied as to the bases, reversed for '-'.  cmgpu_fastq_commit appends names, bases and qualities to a run-wide read
 * store in HBM: per mate, indexed by read_id - read_id_base, 64-bit offsets, geometric growth.  Batches must be committed with
 * consecutive read ids (a gap: CMGPU_EINVAL, nothing is committed); no room in HBM: CMGPU_ENOMEM (the message names the store and its
 * size).  With it on, a record whose quality line is not as long as its sequence (kseq's "truncated quality") makes the scan return
 * CMGPU_EFORMAT; with it off the qualities of reads are not looked at.  Call it before the first scan of a run.  It and
 * cmgpu_fastq_keep_names exclude each other (CMGPU_EINVAL).  Cost: name + 2 x length bytes + 16 bytes of offsets per read. */
int cmgpu_fastq_keep_reads(cmgpu_ctx *ctx, int on);
/* empties the read store (a new run; the next commit sets read_id_base) */
int cmgpu_reads_clear(cmgpu_ctx *ctx);
/* mate: 0 = read 1, 1 = read 2 (n_reads 0 for single-end runs) */
int cmgpu_reads_info(const cmgpu_ctx *ctx, int mate, uint64_t *n_reads, uint64_t *name_bytes, uint64_t *base_bytes, uint32_t *read_id_base);
/* one mate of the read store on the host: names back to back with name_offsets[n_reads + 1], bases and quals (base_bytes each) with
 * offsets[n_reads + 1] -- what the host parser keeps in SequenceBatch (src/sequence_batch.h); for tests and host-side writers */
int cmgpu_download_reads(cmgpu_ctx *ctx, int mate, char *names, uint64_t names_capacity, uint64_t *name_offsets, char *bases, char *quals,
                         uint64_t bases_capacity, uint64_t *offsets);
/* cmgpu_compute_barcode_abundance over the barcodes last taken from stream 2; feed the barcode
 * file in whole reference batches and stop when *done is set (20 M sampled, src/chromap.h:211). */
int cmgpu_barcode_abundance_resident(cmgpu_ctx *ctx, uint64_t *num_sample_barcodes, int *done);

/* ---- --summary: per-barcode mapping statistics ------------------------------------------------
 * Replaces SummaryMetadata (src/summary_metadata.h) and the places that feed it: TOTAL per read batch (src/chromap.h:495-515,
 * 1190-1230) and DUP / LOWMAPQ / MAPPED where duplicates are resolved (src/mapping_writer.h:281-350, 405-437).  The counters live in
 * an open-addressing table in HBM, keyed by the 2-bit packed (corrected) barcode; bulk data counts under key 0.
 *   cmgpu_summary_enable    on != 0: from now on every cmgpu_map_resident (and so every cmgpu_map_* call) counts the batch's reads under
 *                           their barcodes after correction -- a read whose barcode is not on the whitelist goes to the non-whitelist
 *                           counter instead, unless output_mappings_not_in_whitelist -- and cmgpu_store_format / _format_pairs* /
 *                           _format_sam credit every run of duplicates to its survivor's barcode: a run of d records whose survivor has
 *                           MAPQ >= mapq_threshold adds d - 1 to dup, otherwise d to lowmapq; d to mapped either way.  d is the run
 *                           length in low_memory_mode, min(255, run length) otherwise (num_dups_); without remove_pcr_duplicates every
 *                           record is a run.  Each format call adds its store's runs once more: format once per run, or clear.
 *                           Call it after cmgpu_set_whitelist / cmgpu_copy_whitelist (the table is sized from the whitelist; it
 *                           grows by rehash when there is none).  Barcodes of 32 bases: CMGPU_EINVAL at the first batch.  A context
 *                           without it launches exactly the kernels it launched before.
 *   cmgpu_summary_clear     all counters and keys back to empty (a new run)
 *   cmgpu_summary_download  the table's entries in no particular order; first_read_id = the smallest read id counted under the key
 *                           (first_read_id of the batch + index; all ones: the key got records only, from another context of a
 *                           multi-GPU run).  capacity < entries: CMGPU_ECAPACITY with *n_out = the number needed
 *   cmgpu_write_summary     host: the CSV of SummaryMetadata::Output (src/summary_metadata.h:98-128) from the tables of one or more
 *                           contexts (a multi-GPU run: counters of equal keys are added, the smallest first_read_id stands).  Rows come
 *                           in the iteration order of the reference's khash map, which received the keys in first_read_id order;
 *                           halve_pairs != 0 (paired-end --SAM): dup, lowmapq and mapped are halved per barcode
 *                           (AdjustPairedEndOverCount); nonwhitelist_row != 0 (a whitelist was given and unlisted reads are not
 *                           mapped): the "non-whitelist" row ends the file; num_cache_slots_column == 0:
 *                           --turn-off-num-uniq-cache-slots.  barcode_length 0: bulk data, the barcode column is empty.  The
 *                           reference's minimizer cache is not modelled: cachehit and numcacheslots are 0, fric and estfrip 0.00000. */
typedef struct cmgpu_summary_entry {
  uint64_t key;
  uint64_t first_read_id;
  uint32_t total, dup, lowmapq, mapped;
} cmgpu_summary_entry;
typedef struct cmgpu_summary_table {
  const cmgpu_summary_entry *entries;
  uint64_t n_entries;
  uint64_t nonwhitelist_total;
} cmgpu_summary_table;
int cmgpu_summary_enable(cmgpu_ctx *ctx, int on);
int cmgpu_summary_clear(cmgpu_ctx *ctx);
int cmgpu_summary_info(cmgpu_ctx *ctx, uint64_t *n_keys, uint64_t *n_slots);
int cmgpu_summary_download(cmgpu_ctx *ctx, cmgpu_summary_entry *out, uint64_t capacity, uint64_t *n_out, uint64_t *nonwhitelist_total);
/* SAM text written on the host (cmgpu_write_sam*): between _begin and _end the writers called by this thread credit the runs they resolve;
 * _end hands the entries over (total 0, first_read_id all ones) as one more table for cmgpu_write_summary, next to the context's, which
 * holds the reads' TOTAL.  capacity too small: CMGPU_ECAPACITY with *n_out = the number needed, and the collector stays open. */
int cmgpu_host_summary_begin(void);
int cmgpu_host_summary_end(cmgpu_summary_entry *out, uint64_t capacity, uint64_t *n_out);
int cmgpu_write_summary(const cmgpu_summary_table *tables, uint32_t n_tables, uint32_t barcode_length, int nonwhitelist_row,
                        int halve_pairs, int num_cache_slots_column, const char *out_path);

/* Host post-processing that defines the final BED bytes: sort by (rid, operator<),
 * PCR-duplicate removal as in the low-memory merge, MAPQ filter, Tn5 shift, text
 * formatting (src/mapping_writer.h:166-376, src/mapping_writer.cc:72-83). Sorts `records`
 * in place.  names: n_sequences reference names. */
int64_t cmgpu_write_bed_pe(const char *const *names, uint32_t n_sequences, const cmgpu_params *params,
                           cmgpu_record *records, uint64_t n_records, const char *out_path);

/* pairs output of --preset hic (src/mapping_writer.cc:381-420): sort by PairsMapping::operator<
 * (src/pairs_mapping.h:40-43), MAPQ filter, header + one line per record.  read_names[read_id -
 * read_id_base] is the name of read 1 of the pair (host strings; cmgpu_store_format_pairs_resident renders the same lines from the
 * names the device ingest kept). */
int64_t cmgpu_write_pairs(const char *const *names, const uint32_t *lengths, uint32_t n_sequences,
                          const cmgpu_params *params, cmgpu_pairs_record *records, uint64_t n_records,
                          const char *const *read_names, uint32_t read_id_base, const char *out_path);
int64_t cmgpu_write_pairs_ranked(const char *const *names, const uint32_t *lengths, uint32_t n_sequences,
                                 const cmgpu_params *params, cmgpu_pairs_record *records, uint64_t n_records,
                                 const char *const *read_names, uint32_t read_id_base, const uint32_t *pairs_rank,
                                 const char *out_path);

/* Host loaders mirroring Index::Load and SequenceBatch::LoadAllSequences for callers
 * that do not have the reference's own objects (the CLI, Python).  Free with
 * cmgpu_free_host_index / cmgpu_free_host_ref. */
int cmgpu_load_index_file(const char *path, cmgpu_index_view *out);
void cmgpu_free_host_index(cmgpu_index_view *v);
int cmgpu_load_reference_fasta(const char *path, cmgpu_ref_view *out);
void cmgpu_free_host_ref(cmgpu_ref_view *v);

#ifdef __cplusplus
}
#endif
#endif /* CHROMAP_AMD_H_ */
