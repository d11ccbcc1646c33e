// cm_cli_args.h -- the command line of `chromap-amd` (cm_cli.cpp): chromap's flags for the mapping path (chromap_driver.cc:216-761),
// parsed into Args, and the checks that need nothing but the arguments.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/chromap_amd.h"

static void die(const std::string &m);  // (cm_cli.cpp)

// --read-format (Chromap::ParseReadFormat chromap.cc:825-866, SequenceEffectiveRange): per stream up to four
// [start, end] ranges and a strand
struct ReadFormat {
  std::vector<int32_t> starts, ends;
  char strand = '+';
  bool identity() const { return starts.empty() || (strand == '+' && starts[0] == 0 && ends[0] == -1); }
  uint32_t eff_len(uint32_t len) const {
    if (identity()) return len;
    uint32_t out = 0;
    for (size_t k = 0; k < starts.size(); ++k) {
      int st = starts[k], en = ends[k] == -1 ? (int)len - 1 : ends[k];
      if (en >= (int)len) en = (int)len - 1;
      if (st < 0) st = 0;
      if (en >= st) out += (uint32_t)(en - st + 1);
    }
    return out;
  }
  // SequenceEffectiveRange::Replace for the host parser (SAM output, --host-ingest)
  void apply(std::string &seq, std::string &qual) const {
    if (identity()) return;
    std::string ns, nq;
    for (size_t k = 0; k < starts.size(); ++k) {
      int st = starts[k], en = ends[k] == -1 ? (int)seq.size() - 1 : ends[k];
      if (en >= (int)seq.size()) en = (int)seq.size() - 1;
      if (st < 0) st = 0;
      for (int p = st; p <= en; ++p) { ns.push_back(seq[p]); if ((size_t)p < qual.size()) nq.push_back(qual[p]); }
    }
    if (strand == '-') {
      for (char &c : ns) { const char u = c & 0xDF; c = u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N'; }
      std::reverse(ns.begin(), ns.end());
      std::reverse(nq.begin(), nq.end());
    }
    seq.swap(ns);
    qual.swap(nq);
  }
};

struct Args {
  std::string index_path, ref_path, out_path, preset, whitelist, chr_order_path, pairs_order_path, translate_path, summary_path;
  bool summary_cache_slots = true;  // --turn-off-num-uniq-cache-slots clears it
  std::vector<std::string> r1, r2, bc;
  cmgpu_params p;
  bool build_index = false, out_bed = true, out_pairs = false, cell_level_dedup = false, host_ingest = false, out_sam = false, out_tagalign = false, skip_bc_check = false;
  size_t chunk_bytes = 256u << 20;
  bool chunk_given = false;  // (--ingest-chunk-mb: also the size of the pieces of block-compressed input handed to the device)
  ReadFormat fmt[3];  // read 1, read 2, barcode
  int k = 17, w = 7, device = 0, gpus = 1;
  bool force_exchange = false;
  bool output_bgzf = false;  // --output-bgzf: the output file is BGZF blocks, compressed on the device
  bool out_bam = false;      // --BAM: SAM's record route (out_sam), the selected records written as a BAM file (always BGZF)
  bool output_tbi = false;   // --output-tbi: <output>.tbi, the tabix index of the BGZF output, built on the device
  bool output_bai = false;   // --output-bai: <output>.bai, the BAM index of --BAM output, built on the device
  bool output_csi = false;   // --output-csi: <output>.csi, the CSI index of --BAM or BGZF BED / TagAlign output, built on the device
  uint32_t batch_pairs = 4000000;  // multiple of the reference's 500000-pair read batch
};

static std::vector<std::string> split_commas(const std::string &s) {
  std::vector<std::string> v;
  size_t a = 0;
  while (a <= s.size()) {
    size_t b = s.find(',', a);
    if (b == std::string::npos) b = s.size();
    if (b > a) v.push_back(s.substr(a, b - a));
    a = b + 1;
  }
  return v;
}

static Args parse(int argc, char **argv) {
  Args a;
  cmgpu_default_params(&a.p);
  // presets first, explicit flags override (chromap_driver.cc:247-275)
  for (int i = 1; i + 1 < argc; ++i)
    if (!strcmp(argv[i], "--preset")) {
      a.preset = argv[i + 1];
      if (cmgpu_apply_preset(&a.p, argv[i + 1]) != 0) die(std::string("Unrecognized preset parameters ") + argv[i + 1] + "\n");
      if (a.preset == "hic") { a.out_pairs = true; a.out_bed = false; }
      if (a.preset == "atac") a.cell_level_dedup = true;
    }
  for (int i = 1; i + 1 < argc; ++i)
    if (!strcmp(argv[i], "--min-frag-length")) {  // chromap_driver.cc:277-289; -k / -w override it
      const int mfl = atoi(argv[i + 1]);
      if (mfl <= 60) { a.k = 17; a.w = 7; } else if (mfl <= 80) { a.k = 19; a.w = 10; } else { a.k = 23; a.w = 11; }
    }
  for (int i = 1; i < argc; ++i) {
    const std::string o = argv[i];
    auto need = [&](const char *what) -> const char * { if (i + 1 >= argc) die(std::string("missing value for ") + what); return argv[++i]; };
    if (o == "--preset" || o == "--min-frag-length") { ++i; }
    else if (o == "-i" || o == "--build-index") a.build_index = true;
    else if (o == "-x" || o == "--index") a.index_path = need("-x");
    else if (o == "-r" || o == "--ref") a.ref_path = need("-r");
    else if (o == "-o" || o == "--output") a.out_path = need("-o");
    else if (o == "-1" || o == "--read1") a.r1 = split_commas(need("-1"));
    else if (o == "-2" || o == "--read2") a.r2 = split_commas(need("-2"));
    else if (o == "-b" || o == "--barcode") a.bc = split_commas(need("-b"));
    else if (o == "--barcode-whitelist") a.whitelist = need("--barcode-whitelist");
    else if (o == "-k" || o == "--kmer") a.k = atoi(need("-k"));
    else if (o == "-w" || o == "--window") a.w = atoi(need("-w"));
    else if (o == "-e" || o == "--error-threshold") a.p.error_threshold = atoi(need("-e"));
    else if (o == "-s" || o == "--min-num-seeds") a.p.min_num_seeds = atoi(need("-s"));
    else if (o == "-f" || o == "--max-seed-frequencies") {
      auto v = split_commas(need("-f"));
      if (v.size() != 2) die("Positive integers are required for max seed frequencies!");
      a.p.max_seed_frequency0 = atoi(v[0].c_str());
      a.p.max_seed_frequency1 = atoi(v[1].c_str());
    }
    else if (o == "-l" || o == "--max-insert-size") a.p.max_insert_size = atoi(need("-l"));
    else if (o == "-q" || o == "--MAPQ-threshold") a.p.mapq_threshold = atoi(need("-q"));
    else if (o == "-n" || o == "--max-num-best-mappings") a.p.max_num_best_mappings = atoi(need("-n"));
    else if (o == "--min-read-length") a.p.min_read_length = atoi(need("--min-read-length"));
    else if (o == "--drop-repetitive-reads") a.p.drop_repetitive_reads = atoi(need("--drop-repetitive-reads"));
    else if (o == "--bc-error-threshold") a.p.bc_error_threshold = atoi(need("--bc-error-threshold"));
    else if (o == "--bc-probability-threshold") a.p.bc_probability_threshold = atof(need("--bc-probability-threshold"));
    else if (o == "--output-mappings-not-in-whitelist") a.p.output_mappings_not_in_whitelist = 1;
    else if (o == "--trim-adapters") a.p.trim_adapters = 1;
    else if (o == "--remove-pcr-duplicates") a.p.remove_pcr_duplicates = 1;
    else if (o == "--remove-pcr-duplicates-at-cell-level") a.cell_level_dedup = true;
    else if (o == "--remove-pcr-duplicates-at-bulk-level") a.cell_level_dedup = false;
    else if (o == "--Tn5-shift") a.p.tn5_shift = 1;
    else if (o == "--split-alignment") a.p.split_alignment = 1;
    else if (o == "--low-mem") a.p.low_memory_mode = 1;
    else if (o == "--allocate-multi-mappings") a.p.allocate_multi_mappings = 1;
    else if (o == "--multi-mapping-allocation-distance") a.p.multi_mapping_allocation_distance = atoi(need("--multi-mapping-allocation-distance"));
    else if (o == "--multi-mapping-allocation-seed") a.p.multi_mapping_allocation_seed = atoi(need("--multi-mapping-allocation-seed"));
    else if (o == "--BED") { a.out_bed = true; a.out_pairs = false; a.out_sam = false; a.out_bam = false; }
    else if (o == "--SAM") { a.out_sam = true; a.out_bam = false; a.out_bed = false; a.out_pairs = false; }
    else if (o == "--BAM") { a.out_sam = true; a.out_bam = true; a.out_bed = false; a.out_pairs = false; }
    else if (o == "--TagAlign") { a.out_tagalign = true; a.out_bed = true; a.out_sam = false; a.out_bam = false; a.out_pairs = false; }
    else if (o == "--pairs") { a.out_pairs = true; a.out_bed = false; }
    else if (o == "-t" || o == "--num-threads") need("-t");  // host threads are irrelevant here
    else if (o == "--skip-barcode-check") a.skip_bc_check = true;
    else if (o == "--barcode-translate") a.translate_path = need("--barcode-translate");
    else if (o == "--summary") { a.summary_path = need("--summary"); if (a.summary_path.empty()) die("missing value for --summary"); }
    else if (o == "--turn-off-num-uniq-cache-slots") a.summary_cache_slots = false;
    else if (o == "--frip-est-params") {
      // five coefficients separated by ';' (chromap.h:706-727).  They weigh fric, which needs the minimizer cache's hit counts: this build
      // does not model the cache, fric is 0 and estfrip with it, so the values are checked and go no further
      const std::string f = need("--frip-est-params");
      size_t cnt = 0, p0 = 0;
      while (p0 <= f.size() && !f.empty()) {
        size_t p1 = f.find(';', p0);
        if (p1 == std::string::npos) p1 = f.size();
        const std::string tok = f.substr(p0, p1 - p0);
        char *end = nullptr;
        (void)strtod(tok.c_str(), &end);
        if (tok.empty() || end == tok.c_str()) die("--frip-est-params: '" + tok + "' is not a number (five coefficients separated by ';')");
        ++cnt;
        p0 = p1 + 1;
        if (p1 == f.size()) break;
      }
      if (cnt != 5) die("--frip-est-params: invalid number of parameters, expecting 5 parameters but found " + std::to_string(cnt) + " parameters");
    }
    else if (o == "--read-format") {
      const std::string f = need("--read-format");
      size_t at = 0;
      while (at < f.size()) {
        size_t j = f.find(',', at);
        if (j == std::string::npos) j = f.size();
        const std::string tok = f.substr(at, j - at);
        int st = tok.compare(0, 2, "r1") == 0 ? 0 : tok.compare(0, 2, "r2") == 0 ? 1 : tok.compare(0, 2, "bc") == 0 ? 2 : -1;
        if (st < 0 || tok.size() < 4 || tok[2] != ':') die("Unknown read format: " + f + "\n");
        std::vector<std::string> fld;
        size_t p = 3;
        while (p <= tok.size()) { size_t q = tok.find(':', p); if (q == std::string::npos) q = tok.size(); fld.push_back(tok.substr(p, q - p)); p = q + 1; }
        if (fld.size() < 2 || fld.size() > 3) die("Unknown read format: " + f + "\n");
        a.fmt[st].starts.push_back(atoi(fld[0].c_str()));
        a.fmt[st].ends.push_back(atoi(fld[1].c_str()));
        if (fld.size() == 3 && !fld[2].empty()) a.fmt[st].strand = fld[2][0];
        if (a.fmt[st].starts.size() > 4) die("at most four ranges per stream in --read-format");
        at = j + 1;
      }
    }
    else if (o == "--chr-order") a.chr_order_path = need("--chr-order");
    else if (o == "--pairs-natural-chr-order") a.pairs_order_path = need("--pairs-natural-chr-order");
    else if (o == "--device") a.device = atoi(need("--device"));
    else if (o == "--gpus") a.gpus = atoi(need("--gpus"));           // one context + host thread per GPU, records exchanged to chromosome owners
    else if (o == "--force-exchange") a.force_exchange = true;      // the multi-GPU code path with one GPU
    else if (o == "--output-bgzf") a.output_bgzf = true;
    else if (o == "--output-tbi") a.output_tbi = true;
    else if (o == "--output-bai") a.output_bai = true;
    else if (o == "--output-csi") a.output_csi = true;
    else if (o == "--host-ingest") a.host_ingest = true;   // kseq-style host parser (the fallback for text the device ingest refuses)
    else if (o == "--ingest-chunk-mb") { a.chunk_bytes = (size_t)atol(need("--ingest-chunk-mb")) << 20; a.chunk_given = true; }
    else if (o == "--batch-pairs") a.batch_pairs = (uint32_t)atol(need("--batch-pairs"));
    else if (o == "-v" || o == "--version") { printf("chromap-amd 0.1 (hot path of chromap 0.3.3-r521 on gfx950)\n"); exit(0); }
    else if (o == "-h" || o == "--help") {
      printf("Usage: chromap-amd -i -r ref.fa -o index | chromap-amd [--preset atac|chip|hic] -x index -r ref.fa -1 r1.fq[.gz] [-2 r2.fq[.gz]]\n"
             "       [-b barcode.fq --barcode-whitelist wl.txt] -o out [-e -s -f -l -q --min-read-length --trim-adapters\n"
             "       --remove-pcr-duplicates --Tn5-shift --low-mem --BED|--TagAlign|--pairs|--SAM|--BAM --bc-error-threshold ...]\n"
             "       [--summary FILE [--turn-off-num-uniq-cache-slots] [--frip-est-params a;b;c;d;e]]\n"
             "  --allocate-multi-mappings  BED / TagAlign without --low-mem and without a preset: every read whose mappings have MAPQ < 4 is given to\n"
             "                  one of them, drawn by the uniquely mapped fragments around each; reads with none around are dropped\n"
             "  --multi-mapping-allocation-distance INT  how far around a mapping the uniquely mapped fragments count [0]\n"
             "  --multi-mapping-allocation-seed INT      seed of the draw [11]\n"
             "  --split-alignment  with -1 alone (single-end reads): BED, --TagAlign or --SAM whose coordinates and MAPQ carry each read's split site;\n"
             "                  with -2 as well the output is --pairs (--preset hic)\n"
             "  --barcode-translate FILE  lines to<TAB or ,>from (gzip or plain): BED column 4 and the SAM CB:Z: value are written as the\n"
             "                  table's names; BED is translated on the device, --SAM on the host\n"
             "  --BAM           the records of --SAM as a BAM file (@SQ header, NM / MD / CB tags), encoded and BGZF-compressed on the device; one\n"
             "                  GPU, device ingest; its index: --output-bai, --output-csi.  Not with --host-ingest, --barcode-translate, -n > 1, --output-tbi\n"
             "  --output-bgzf   the output file as BGZF blocks (bgzip's format, readable by tabix / pairix / samtools), compressed on the\n"
             "                  device; nothing is inferred from the output file's name.  Not where the host renders the text:\n"
             "                  --host-ingest --SAM, --SAM --barcode-translate\n"
             "  --output-tbi    with --output-bgzf and BED or single-end --TagAlign output on one GPU: the tabix index of the output file\n"
             "                  (what `tabix -p bed` would make of it), built on the device and written to <output>.tbi\n"
             "  --output-bai    with --BAM: the BAM index of the output file (what `samtools index` would make of it, bins not folded), built\n"
             "                  on the device and written to <output>.bai\n"
             "  --output-csi    with --BAM, or with --output-bgzf and BED or single-end --TagAlign output on one GPU: the CSI index of the output\n"
             "                  file (what `samtools index -c` / `tabix -C -p bed` would make of it, bins not folded), built on the device and\n"
             "                  written to <output>.csi; the one index for a chromosome longer than 2^29 bases (min_shift 14, depth 5, or 6\n"
             "                  with such a chromosome).  Allowed beside --output-tbi / --output-bai\n"
             "  --summary FILE  per-barcode CSV (one row for bulk data): barcode,total,duplicate,unmapped,lowmapq counted on the device;\n"
             "                  cachehit, fric, estfrip and numcacheslots are written as 0 (the minimizer cache is not modelled)\n");
      exit(0);
    }
    else die("unsupported option " + o + " (PAF output is outside this build)");
  }
  if (a.p.max_num_best_mappings > a.p.drop_repetitive_reads) {  // chromap_driver.cc:630-641
    fprintf(stderr, "WARNING: you want to drop mapped reads with more than %d mappings. But you want to output top %d best mappings. "
                    "In this case, only reads with <=%d best mappings will be output.\n",
            a.p.drop_repetitive_reads, a.p.max_num_best_mappings, a.p.drop_repetitive_reads);
    a.p.max_num_best_mappings = a.p.drop_repetitive_reads;
  }
  if (a.p.max_num_best_mappings < 1) die("-n must be at least 1");
  // every pair of a batch has -n record slots in HBM (24 + 5 bytes each), addressed with 32 bits: large -n values map smaller batches (whole
  // reference batches of 500 000 pairs, so that the multi-mappers' sampling is the reference's); beyond 8192 one reference batch has more
  // than 2^32 slots
  if (a.p.max_num_best_mappings > 8192) die("-n above 8192 is outside this build (a 500000-pair batch then needs more than 2^32 record slots)");
  // (the reference counts MAPPED per mapping there and prints total - mapped as an unsigned number that wraps: nothing to reproduce)
  if (!a.summary_path.empty() && a.p.max_num_best_mappings > 1) die("--summary with -n > 1 is outside this build");
  if (a.out_bam) a.output_bgzf = true;  // (a BAM file is a BGZF stream: --output-bgzf beside --BAM changes nothing)
  if (a.out_sam) {
    if (a.out_bam && a.p.max_num_best_mappings > 1) die("--BAM with -n > 1 is outside this build");
    if (a.p.max_num_best_mappings > 1) die("--SAM with -n > 1 is outside this build");
    a.p.output_format = CMGPU_FORMAT_SAM;
  }
  // the reference accepts these combinations; this build has no record type for them -- refuse instead of writing garbage
  if (a.out_pairs && !a.p.split_alignment) a.p.output_format = CMGPU_FORMAT_PAIRS;  // MapPairedEndReads<PairsMapping> on the ordinary pairing (chromap_driver.cc:748-751)
  if (a.gpus < 1 || a.gpus > 64) die("--gpus must be 1..64");
  if (a.p.max_num_best_mappings > 64) {
    const uint64_t budget = 1ull << 30;  // record slots per batch (31 GB of HBM)
    const uint64_t fit = budget / (uint64_t)a.p.max_num_best_mappings;
    if (a.batch_pairs > fit) a.batch_pairs = (uint32_t)fit;
  }
  if (a.batch_pairs < 500000) a.batch_pairs = 500000;
  a.batch_pairs -= a.batch_pairs % 500000;
  return a;
}

// Everything that can be said about an invocation from its arguments alone, before any file is opened (or emptied) and before a GPU
// is touched.  Sets dedup_at_bulk_level.
static void validate(Args &a) {
  if (a.ref_path.empty() || a.out_path.empty()) die("No reference / output specified!");
  if (a.build_index) return;
  if (a.index_path.empty() || a.r1.empty()) die("No index / read files specified!");
  const bool paired = !a.r2.empty(), barcoded = !a.bc.empty();
  if (a.out_pairs && !paired) die("No support for single-end HiC yet!");  // chromap_driver.cc:716-718
  if (paired && a.r1.size() != a.r2.size()) die("Numbers of read1 and read2 files don't match!");
  if (barcoded && a.bc.size() != a.r1.size()) die("Numbers of read1 and barcode files don't match!");
  if (barcoded && a.whitelist.empty() && a.p.remove_pcr_duplicates && a.p.low_memory_mode && !a.cell_level_dedup)
    die("bulk-level duplicate removal ranks barcodes by whitelist abundance: give --barcode-whitelist or --remove-pcr-duplicates-at-cell-level");
  a.p.dedup_at_bulk_level = barcoded && !a.cell_level_dedup ? 1 : 0;  // remove_pcr_duplicates_at_bulk_level defaults to true (mapping_parameters.h:49)
  if (a.output_bai && !a.out_bam) die("--output-bai needs --BAM (the index is that of a BAM file's records)");
  // BAM records are encoded from one context's stores in HBM and leave through the BGZF writer
  if (a.out_bam) {
    if (a.host_ingest) die("--BAM with --host-ingest is outside this build (the host renders that output, as SAM text; convert it with samtools view -b)");
    if (!a.translate_path.empty())
      die("--BAM with --barcode-translate is outside this build (the command line's route for it is the host writer, which renders SAM text)");
    if (a.output_tbi) die("--output-tbi with --BAM is outside this build (BAM takes a .bai index: --output-bai)");
    if (a.gpus > 1 || a.force_exchange) die("--BAM with --gpus > 1 or --force-exchange is outside this build (the records are encoded by one context from its own stores)");
    if (a.p.allocate_multi_mappings && !a.p.low_memory_mode)
      die("--allocate-multi-mappings with --BAM is outside this build (the SAM and BAM writers have no allocation stage)");
  }
  if ((a.gpus > 1 || a.force_exchange) && (a.out_pairs || a.out_sam || a.host_ingest))
    die("--gpus > 1 needs BED / TagAlign output and device-side FASTQ ingest (pairs and SAM text is rendered by one context from its own stores)");
  // the compressor reads the text store in HBM; the host SAM writers render into a file
  if (a.output_bgzf && a.out_sam && a.host_ingest) die("--output-bgzf with --host-ingest --SAM is outside this build (the host renders that text; compress the file with bgzip)");
  if (a.output_bgzf && a.out_sam && !a.translate_path.empty())
    die("--output-bgzf with --SAM --barcode-translate is outside this build (the host renders that text; compress the file with bgzip)");
  // the index is made of one context's sorted BED text and its blocks
  if (a.output_tbi) {
    if (!a.output_bgzf) die("--output-tbi needs --output-bgzf (the index is that of the BGZF blocks)");
    if (a.out_sam) die("--output-tbi with --SAM is outside this build (a tabix index of SAM text; --BAM --output-bai writes BAM and its index)");
    if (a.out_pairs) die("--output-tbi with pairs output is outside this build (pairs text takes a .px2 index, which is not built)");
    if (a.out_tagalign && paired) die("--output-tbi with paired-end --TagAlign is outside this build (two lines per pair: the text is not sorted by start)");
    if (a.gpus > 1 || a.force_exchange) die("--output-tbi with --gpus > 1 or --force-exchange is outside this build (the output has one section per GPU)");
  }
  // ... or of one context's BAM records
  if (a.output_csi) {
    if (!a.output_bgzf) die("--output-csi needs --BAM or --output-bgzf (the index is that of the BGZF blocks)");
    if (a.out_sam && !a.out_bam) die("--output-csi with --SAM is outside this build (a CSI index of SAM text; --BAM --output-csi writes BAM and its index)");
    if (a.out_pairs) die("--output-csi with pairs output is outside this build (pairs text takes a .px2 index, which is not built)");
    if (a.out_tagalign && paired) die("--output-csi with paired-end --TagAlign is outside this build (two lines per pair: the text is not sorted by start)");
    if (a.gpus > 1 || a.force_exchange) die("--output-csi with --gpus > 1 or --force-exchange is outside this build (the output has one section per GPU)");
  }
  // the reference allocates in its in-memory flavour only (chromap.h:1305-1353): with --low-mem or a preset the flag does nothing there and here
  if (a.p.allocate_multi_mappings && !a.p.low_memory_mode) {
    if (a.out_sam) die("--allocate-multi-mappings with --SAM is outside this build (the SAM writers have no allocation stage)");
    if (a.out_pairs) die("--allocate-multi-mappings with pairs output is outside this build (the pairs writers have no allocation stage)");
    if (!a.summary_path.empty()) die("--allocate-multi-mappings with --summary is outside this build (the duplicate and low-MAPQ counts are taken before the allocation)");
    if (a.gpus > 1 || a.force_exchange)
      die("--allocate-multi-mappings with --gpus > 1 or --force-exchange is outside this build (a read's positions lie on chromosomes that different GPUs own)");
  }
}
