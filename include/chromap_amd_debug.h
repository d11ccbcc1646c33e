/* chromap_amd_debug.h -- measurement, test and fixture hooks of libchromap_amd.so.
 *
 * NOT part of the drop-in boundary (include/chromap_amd.h holds SURVEY.md 8(b)'s contract: create / map / wait / destroy,
 * the writers and the post-processing a maintainer binds).  What is declared here exists for bench.py, the parity tests and
 * the profiling tools: synthetic genomes and read batches generated on the device, the kernel-only probe measurement,
 * measurement knobs, stage-level views of the last mapped batch and exports of the resident index / reference for the
 * oracle.  Plain C like the boundary header.
 *
 * Environment variables the library / CLI read (measurement and test aids, no effect on results):
 *   CM_NO_KEY32     the cooperative hit-list stage keeps the reference's 64-bit keys although the reference would fit 32-bit
 *                   global coordinates (the path of references beyond 4 Gbases; tests/test_gpu_stages.py)
 *   CM_DEBUG_POOL   per mapped range: size of and demand on the rescue-hit pool, time of its (re)allocation, on stderr
 *   CM_CLI_TIMES    chromap-amd: seconds of every scan / take + commit / map / store call on stderr
 */
#ifndef CHROMAP_AMD_DEBUG_H_
#define CHROMAP_AMD_DEBUG_H_

#include "chromap_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bench/test helper standing in for Index::Construct (src/index.cc:12-89) on a synthetic
 * genome: n_sequences chromosomes of uniform random bases (xorshift seeded with seed) are
 * generated and indexed on the device (functionally identical lookup results; bucket
 * placement differs from khash's).  total_bases may be GRCh38-sized (3.1e9). */
int cmgpu_create_synthetic(uint64_t total_bases, uint32_t n_sequences, uint64_t seed, int32_t kmer_size,
                           int32_t window_size, const cmgpu_params *params, int device_id, cmgpu_ctx **out);

/* The same with planted repeat families: n_families elements of element_len random bases, `copies`
 * copies each, spread over the genome in either orientation, every copy's bases replaced with probability
 * `divergence` -- so that frequent seeds, multi-mappers and mate rescue occur as on a real genome. */
int cmgpu_create_synthetic_repeats(uint64_t total_bases, uint32_t n_sequences, uint64_t seed, int32_t kmer_size,
                                   int32_t window_size, const cmgpu_params *params, int device_id, uint32_t n_families,
                                   uint32_t copies, uint32_t element_len, double divergence, cmgpu_ctx **out);

/* The same with a whole repeat landscape instead of one family class.  profile 1: 64-kb tiles, 20 % of them packed with
 * SINE-like 300-base elements (128 families, ~10^4 copies each on 3.1 Gb, 5-15 % divergence per copy), 12 % with LINE-like
 * 3-kb elements (256 families, ~360 copies each, 1-5 %), 2 % satellite arrays (171-base units, 2 % replaced): 22.5 % of the
 * bases are repeat-derived (bench.py's third workload).  profile 2: the same kinds with 40 % / 28 % / 3 % of the tiles: 47 % of
 * the bases repeat-derived (~19 000 copies per SINE-like family, ~830 per LINE-like family): bench.py's fourth genome. */
int cmgpu_create_synthetic_profile(uint64_t total_bases, uint32_t n_sequences, uint64_t seed, int32_t kmer_size,
                                   int32_t window_size, const cmgpu_params *params, int device_id, uint32_t profile,
                                   cmgpu_ctx **out);

/* Generates n_pairs synthetic read pairs from the ctx's reference directly in HBM
 * (fragment length uniform in [frag_min, frag_max), substitution rate sub_rate, R1/R2
 * swapped with p = 0.5) and makes them the resident batch. */
int cmgpu_generate_resident_batch(cmgpu_ctx *ctx, uint32_t n_pairs, uint32_t read_length, uint32_t frag_min,
                                  uint32_t frag_max, double sub_rate, uint64_t seed);
/* The same with 1-base insertions / deletions at rate indel_rate per base (half each). */
int cmgpu_generate_resident_batch_indels(cmgpu_ctx *ctx, uint32_t n_pairs, uint32_t read_length, uint32_t frag_min,
                                         uint32_t frag_max, double sub_rate, double indel_rate, uint64_t seed);
/* Hi-C shaped pairs (BASELINE config 5): the mates come from two independent loci (60 % within 1 Mb on one sequence, the
 * others anywhere), either orientation each; `chimeric_fraction` of the pairs carry a ligation junction inside one read
 * (25 .. L - 25 bases of its own locus, then the partner's fragment on the other strand) -- the input split alignment
 * (draft_mapping_generator.cc:410-487, alignment.cc:197-376) is for. */
int cmgpu_generate_resident_batch_hic(cmgpu_ctx *ctx, uint32_t n_pairs, uint32_t read_length, double sub_rate, double indel_rate,
                                      double chimeric_fraction, uint64_t seed);
/* The resident batch changes places with the one parked in `slot` (0..7; either may be empty): several distinct
 * batches stay in HBM and take turns (the measurement must not map one batch over and over). */
int cmgpu_swap_resident_batch(cmgpu_ctx *ctx, int slot);
/* Copies the resident batch back to host SoA buffers (for checking against the oracle). */
int cmgpu_download_batch(cmgpu_ctx *ctx, char *read1_bases, uint32_t *read1_offsets, char *read2_bases,
                         uint32_t *read2_offsets);

/* Kernel-level entry for the graded index-probe kernel: looks up n minimizer hashes
 * (device-resident after the call) `repeat` times; returns average kernel time in ms
 * measured with HIP events on the launch stream, and the probe-step / hit counts. */
int cmgpu_probe_bench(cmgpu_ctx *ctx, const uint64_t *hashes, uint64_t n, int repeat, double *avg_ms,
                      uint64_t *probe_steps, uint64_t *hits, uint64_t *occurrences);

/* The same kernel in its other shapes, on the hashes left resident by the last mapped batch:
 * lookups_per_lane 1 / 2 / 4 / 8 independent lookups interleaved per lane, pair_prefetch != 0: the second
 * probe step is requested with the first when both buckets share a 64-byte sector. */
int cmgpu_probe_bench_variant(cmgpu_ctx *ctx, uint64_t n, int repeat, int lookups_per_lane, int pair_prefetch,
                              double *avg_ms, uint64_t *probe_steps, uint64_t *hits);

/* The same kernel once, with its answer per hash (tests/test_gpu_index_build.py compares it with kh_get key by key): n hashes
 * from host memory (a minimizer's hash, i.e. the table key >> 1) go through k_probe<lookups_per_lane, pair_prefetch>
 * (lookups_per_lane 1 / 2 / 4 / 8, pair_prefetch 0 / 1) over the file-layout table (file_table != 0) or the table the pipeline
 * probes (file_table == 0: the re-hashed one of "probe_table_shift" when resident).  kind_out[i] is one of the three values
 * below and value_out[i] the bucket's value (0 for a miss); *probe_steps / *hits are the launch's totals (buckets visited as
 * kh_get counts them, hashes found).  Both output arrays hold `capacity` >= n entries: the device arrays are filled with 0xEE
 * bytes over all of them before the launch and all of them come back, so entries past n show whether the kernel kept to n. */
#define CMGPU_PROBE_MISS 0       /* kh_get returns kh_end: an empty bucket ended the walk, or it came round */
#define CMGPU_PROBE_SINGLETON 1  /* the key's low bit is set: the value is the one hit (index_utils.h:56-58) */
#define CMGPU_PROBE_MULTI 2      /* the value is (offset into the occurrence table) << 32 | count (index_utils.h:28-31) */
int cmgpu_debug_probe(cmgpu_ctx *ctx, const uint64_t *hashes, uint64_t n, int lookups_per_lane, int pair_prefetch, int file_table,
                      uint64_t capacity, uint8_t *kind_out, uint64_t *value_out, uint64_t *probe_steps, uint64_t *hits);

/* HBM random-gather microbenchmark on the resident table: n independent 16-byte loads at
 * pseudo-random buckets, average kernel time over `repeat` launches (HIP events). */
int cmgpu_gather_bench(cmgpu_ctx *ctx, uint64_t n, int repeat, double *avg_ms);
/* its sweep: loads_per_lane (1, 2, 4, 8, 16) requests in flight per lane, access_bytes 16 (one bucket) or
 * 64 (the whole aligned sector, every fetched byte used) -- the best shape is the ceiling k_probe is held to */
int cmgpu_gather_sweep(cmgpu_ctx *ctx, uint64_t n, int repeat, int loads_per_lane, int access_bytes, double *avg_ms);

/* Measurement knobs (the defaults are the measured best): "probe_lookups_per_lane" 1/2/4/8,
 * "probe_pair_prefetch" 0/1, "mm_chunks" 1..8, "prep_kernel" 0/1, "item_limit" (largest dense
 * intermediate array, in entries; batches that need more are mapped in sub-batches), "heavy_wave_max" /
 * "heavy_block_max" / "heavy_big_max" (size classes of the cooperative kernel for long hit lists; -1 on the first:
 * one-lane path), "heavy_last" (reads with long hit lists processed in waves of their own: 0 auto, 1 always, -1 never),
 * "lanes" 1..8 (ranges of a batch mapped side by side), "h2d_copy_blocks" / "d2h_copy_blocks" (blocks of the copy kernel
 * that moves page-locked host memory over the link instead of the copy engine; 0 = hipMemcpyAsync),
 * "first_read_id" (read id of the resident batch's first pair; device-generated batches start at 0),
 * "probe_table_shift" 0..4 (the pipeline probes a device copy of the index table re-hashed into 2^shift times as many
 * buckets: same lookups, fewer buckets visited; 0 = the file's table), "coop" (bit mask of the stages whose long lists go to
 * groups of lanes: 1 hit lists, 2 rescue hits, 4 pair filter, 8 acceptance, 16 pairing; 0 = the one-lane / bitonic forms),
 * "speculative_sizes" 0/1 (candidate arrays sized from the previous batch, checked on the device, one re-run when too small; the
 * kernels of the long-list classes launched for the classes the previous range used, one re-run when another class has items; -1: on,
 * starting from an empty launch set -- the tests' way to force that re-run),
 * "verify_planes" 0/1 (alignments of the verification on bit planes of the reference and the reads instead of their bytes),
 * "long_read_fused" 0/1 (reads longer than 69 bases: trimming + minimizers in one pass instead of count / scan / fill),
 * "generic_kernels" 0/1 (1: paired-end batches without split alignment run the S4-S6 kernels that carry every mode instead of
 * their own instances; tests/test_gpu_mode_instances.py compares the two),
 * "s3b_short" 1/0 (0: hit lists of at most 16 hits at a lane cap of 16 go through the general per-lane kernel, k_s3b_candidates,
 * instead of the short-list instance k_s3b_short; tests/test_gpu_s3b_short.py compares the two),
 * "pack_once" 1/0 (batches whose longest read has at most 64 bases, on the fused trim + minimizer kernel: 1 converts every read to
 * bit planes once, in that kernel, for the trim, the minimizer pass and the verification's planes; 0 converts the bytes in each of
 * the three, the last in a kernel of its own, k_pack_reads; tests/test_gpu_pack_once.py compares the two),
 * "s6_planes" 1/0 (1: the pairing stage's start positions count the mismatches in front of the traceback on bit planes for reads of
 * at most 64 bases made of upper-case A/C/G/T only; 0: on bytes for every read; tests/test_gpu_s6_planes.py compares the two).
 * Every setting gives the same records (tests/test_gpu_parity.py runs the fuzz data under each; "s3b_short" 1 and 0:
 * tests/test_gpu_s3b_short.py, on its own data and on one fuzz configuration). */
int cmgpu_set_option(cmgpu_ctx *ctx, const char *name, int64_t value);
int cmgpu_get_option(const cmgpu_ctx *ctx, const char *name, int64_t *value);

/* ---- stage-level view of the last mapped batch (parity tests of the gfx950 build against the oracle's trace) ----
 * cmgpu_trace has the layout of oracle/chromap_oracle.h: ora_trace: per pair the read lengths after trimming
 * (chromap.cc:176-289), minimizer counts (minimizer_generator.cc:7-139), candidates entering verification
 * (candidate_processor.cc:12-263), draft mappings and error bookkeeping (draft_mapping_generator.cc:9-557),
 * pairing (mapping_generator.h:160-253).  Paired-end batches mapped in one piece only. */
typedef struct cmgpu_trace {
  uint32_t len1, len2, n_mm1, n_mm2, n_cand1, n_cand2, n_draft1, n_draft2;
  int32_t min_err1, min_err2, nbest1, nbest2, second1, second2, nsecond1, nsecond2;
  uint32_t rep1, rep2;
  int32_t min_sum, nbest, second_sum, nsecond, force_mapq;
} cmgpu_trace;
int cmgpu_debug_trace(cmgpu_ctx *ctx, cmgpu_trace *out, uint64_t capacity);
/* minimizers of one read (index 2 * pair + mate) / of all reads of the last mapped batch: hash and position << 1 | strand */
int cmgpu_debug_minimizers(cmgpu_ctx *ctx, uint32_t read, uint64_t *hash_out, uint32_t *ps_out, uint32_t capacity, uint32_t *n_out);
int cmgpu_debug_minimizers_all(cmgpu_ctx *ctx, uint32_t *cnt_out, uint32_t *off_out, uint64_t *hash_out, uint32_t *ps_out,
                               uint64_t capacity, uint64_t *n_total);

/* Per-stage timing of the last cmgpu_map_* call (HIP events on the launch stream).
 * names/ms arrays of capacity cap; returns number of stages. */
int cmgpu_last_timings(const cmgpu_ctx *ctx, const char **names, float *ms, int cap);

/* Export of the synthetic reference / index for checking against the oracle (small sizes). */
int cmgpu_export_reference(cmgpu_ctx *ctx, uint32_t seq, char *out, uint32_t capacity);
int cmgpu_reference_lengths(cmgpu_ctx *ctx, uint32_t *lengths, uint32_t capacity, uint32_t *n_sequences);


/* A per-read (2 n entries: "rlen", "mm_cnt", "hit_tot", "ncp", "ncn", "resc_p", "resc_n", "mcp", "mcn", "fcp", "fcn", "ndp",
 * "ndn", "nv") or per-pair (n entries: "pe_nbest") 32-bit array of the last mapped batch -- the list lengths the stages saw
 * (tools/list_hist.py).  *n_out = entries.
 * "hv_cnt": the 64 counters of the device work lists of the last mapped range -- word l < 32 = the reads / pairs that went to
 * long-list class l (the CmList ids of cm_types.h), the words above are the lists' work cursors.  A read-only copy.
 * "read_pl": the reads' bit planes as the verification saw them, for a batch mapped in one piece: S = (6 W + 3) & ~3 words per read,
 * W = (longest read + 31) / 32; read r's forward p0 / p1 / pn (W words each), then the reverse complement's, at r * S.  Defined
 * for reads with rlen > 0; *n_out = 2 n S.
 * "read_plain": per read (2 n entries), for a batch mapped in one piece with "s6_planes" on: 1 when every byte of the raw read is an
 * upper-case A, C, G or T and the front end's planes instance handled the batch, else 0 (one byte per read on the device). */
int cmgpu_debug_array(cmgpu_ctx *ctx, const char *name, uint32_t *out, uint64_t capacity, uint64_t *n_out);

/* ---- the MAPQ functions on their own (tests/test_gpu_mapq.py) ----
 * n cases, one lane each, through the stage functions the mapping path calls (GetMAPQForSingleEndRead / GetMAPQForPairedEndRead,
 * mapping_generator.h:920-1192), with the context's two lookup tables as they stand in HBM.  Case i is pair i with reads 2 i and
 * 2 i + 1; the single-read kinds look at read 2 i only.  The cases are two column-major int32 matrices in host memory:
 *   reads  9 columns of 2 n values: num_errors, alignment_length (< 65536), read_length, min_num_errors, second_min_num_errors,
 *          num_best_mappings, num_second_best_mappings, repetitive_seed_length, candidates on the mapping's strand (split kinds)
 *   pairs  6 columns of n values: max_num_error_difference (single-read kinds), then the pair's min_sum_errors,
 *          second_min_sum_errors, num_best_mappings, num_second_best_mappings and force_mapq (CMGPU_MAPQ_PAIRED)
 * error_threshold is the -e the split kinds read.  out: n bytes, the MAPQ as the record would carry it.  Arguments for which the
 * reference's arithmetic is undefined (a length of 0, a division by num_second_best_mappings / diff + 1 == 0) are the caller's to
 * leave out.  The call reads and writes nothing of the mapped batch and needs none. */
#define CMGPU_MAPQ_SINGLE 0        /* cm_mapq_single: single-end and paired-end reads without split alignment */
#define CMGPU_MAPQ_SPLIT 1         /* cm_mapq_single_split */
#define CMGPU_MAPQ_PAIRED 2        /* cm_mapq_paired */
#define CMGPU_MAPQ_PAIRED_SPLIT 3  /* cm_mapq_paired_split: the pair's value under --split-alignment */
int cmgpu_debug_mapq(cmgpu_ctx *ctx, int kind, int32_t error_threshold, uint64_t n, const int32_t *reads, const int32_t *pairs,
                     uint8_t *out);
/* The two tables themselves, downloaded: len_coef (65536 doubles: a < 50 ? 1 : 3 / log(a)) and nsec_break (*n_break entries:
 * nsec_break[v] = the smallest n >= 1 with (int)(4.343 * log(n + 1) + 0.499) >= v).  Either array may be NULL. */
int cmgpu_debug_mapq_tables(cmgpu_ctx *ctx, double *len_coef, uint32_t *nsec_break, uint32_t capacity, uint32_t *n_break);

#ifdef __cplusplus
}
#endif
#endif /* CHROMAP_AMD_DEBUG_H_ */
