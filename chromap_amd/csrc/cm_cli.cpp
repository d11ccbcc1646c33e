// cm_cli.cpp -- `chromap-amd`: command-line host with chromap's flags for the mapping path
// (chromap_driver.cc:216-761), driving the HIP path through the C ABI.  Host work only:
// argument parsing (cm_cli_args.h), FASTQ(.gz) ingest into SoA batches (cm_cli_reader.h; whole multiples of the reference's
// 500000-pair read batch), statistics, and the post-processing that writes BED / pairs / SAM.  main() at the end lists the stages.
#include <sched.h>

#include <chrono>
#include <functional>

#include "../../include/chromap_amd_debug.h"
#include "cm_cli_reader.h"
#include "cm_cli_args.h"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The processors this process may really use: what the hardware reports, cut to the affinity mask and to the control group's CPU quota.
// (Round 6: the measurement boxes report 256 hardware threads and run the job in a container with a quota of 16 CPUs -- cpu.max
//  "1600000 100000".  Teams sized from the 256 -- 2 x 32 inflating threads, as many again finishing -- used the quota up early in every 100 ms
//  period and the kernel then stopped ALL of the process's threads until the period ended: 155 of 837 periods throttled, 60-90 ms stalls in the
//  middle of 7 ms jobs, and "more threads" made everything slower.)
static unsigned cpu_budget() {
  static const unsigned budget = []() {
    unsigned n = std::thread::hardware_concurrency();
    if (!n) n = 8;
    cpu_set_t set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0 && (unsigned)c < n) n = (unsigned)c; }
    double quota = 0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota us | max> <period us>"
      char q[64];
      double per = 0;
      if (fscanf(f, "%63s %lf", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) quota = atof(q) / per;
      fclose(f);
    } else {  // cgroup v1
      double qu = 0, per = 0;
      if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (fscanf(g, "%lf", &qu) != 1) qu = 0; fclose(g); }
      if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(g, "%lf", &per) != 1) per = 0; fclose(g); }
      if (qu > 0 && per > 0) quota = qu / per;
    }
    if (quota >= 1 && quota < (double)n) n = (unsigned)quota;
    if (const char *e = getenv("CM_CPU_BUDGET")) { const int v = atoi(e); if (v > 0) n = (unsigned)v; }
    return n < 2 ? 2u : n;
  }();
  return budget;
}

static void die(const std::string &m) {  // ExitWithMessage (utils.h:71-74)
  fprintf(stderr, "%s\n", m.c_str());
  // (_exit: other threads of the process may be inside the HIP runtime -- the warm-up beside the index read, the worker mapping the last batch
  //  while this thread found the next one damaged -- and exit() would run the runtime's teardown under them)
  fflush(stdout);
  fflush(stderr);
  _exit(255);
}
// what the reference says about input it cannot read to the end (kseq's negative return values), with this build's reason behind it
static const char kCorrupt[] = "Didn't reach the end of sequence file, which might be corrupted!";
static void die_corrupt(const std::string &detail) { die(std::string(kCorrupt) + " (" + detail + ")"); }

// fn(0) .. fn(n - 1) at the same time, each on a thread of its own -- `first_here`: fn(0) on the calling thread
static void run_side_by_side(int n, bool first_here, const std::function<void(int)> &fn) {
  std::vector<std::thread> th;
  for (int i = first_here ? 1 : 0; i < n; ++i) th.emplace_back(fn, i);
  if (first_here) fn(0);
  for (std::thread &t : th) t.join();
}

// --SAM on the host route (--host-ingest, --barcode-translate): everything the final sort needs, over all batches
struct HostSam {
  std::vector<cmgpu_sam_record> rec;
  std::vector<uint32_t> cigar, md_caps, o1{0}, o2{0};
  std::vector<std::vector<char>> md_batches;
  std::vector<uint64_t> batch_slots, bc;
  std::vector<std::string> names1, names2;
  std::vector<char> b1, q1, b2, q2;
};
// What the stages of a run share
struct Run {
  Args a;
  bool times = false;  // CM_CLI_TIMES: the [times] lines on stderr
  cmgpu_ref_view ref;
  std::vector<cmgpu_ctx *> ctxs;  // one context (index + reference resident, own streams) per GPU; ctxs[0] also runs every single-GPU path
  std::vector<const char *> out_names;  // names / lengths for the writers, in --chr-order
  std::vector<uint32_t> out_lengths, pairs_rank;
  bool paired = false, barcoded = false, exchange = false, device_ingest = false, sam_device = false;
  uint32_t bc_len = 0, next_read_id = 0;
  uint64_t num_reads = 0;
  cmgpu_stats st;
  double t_begin = 0, t_read = 0, t_parse = 0, t_map = 0, t_post = 0;
  double t_compress = 0;       // --output-bgzf: the contexts' compress calls
  uint64_t bgzf_bytes = 0, bgzf_text_bytes = 0;  // --output-bgzf: bytes written (header blocks and the end-of-file block included) for that many bytes of text
  std::vector<std::string> read_names;  // pairs output needs read-1 names by read_id (host parser only: the device ingest keeps them in HBM)
  HostSam sam;
  cmgpu_ctx *ctx() const { return ctxs[0]; }
  bool whitelisted() const { return barcoded && !a.whitelist.empty(); }
};
static void ck(cmgpu_ctx *cx, int rc) { if (rc != CMGPU_OK) die(cmgpu_last_error(cx)); }

// The HIP runtime and the library's device code come up on a thread of their own while the main thread reads the reference and the index
// (an error, e.g. no device, is reported by cmgpu_create).  The output file is opened and emptied there too (the reference opens its
// output before it reads a read, chromap.h:277 / :777 -- the MappingWriter is constructed ahead of the loop): a path that cannot be written
// fails now, not after the mapping, and emptying an existing file of the last run's size -- tens of milliseconds per few hundred MB of
// page cache -- is not left for the moment the text is ready.  Started after validate(): a refused invocation empties nothing.
struct Warm {
  std::thread th;
  bool out_opened = true;
  void start(const Args &a) {
    const bool text_out = !a.build_index && !a.out_pairs && !a.out_sam;
    const int dev0 = a.device, ndev = a.gpus;
    const std::string outp = a.out_path;
    th = std::thread([this, dev0, ndev, text_out, outp]() {
      if (text_out) { FILE *of = fopen(outp.c_str(), "wb"); if (of) fclose(of); else out_opened = false; }
      for (int gi = 0; gi < ndev; ++gi) (void)cmgpu_warm_up(dev0 + gi);
    });
  }
  void join() { if (th.joinable()) th.join(); }
  ~Warm() { join(); }
};
static int build_index(Run &r, Warm &warm) {
  cmgpu_ctx *bctx = nullptr;
  warm.join();
  if (cmgpu_create_from_reference(&r.ref, r.a.k, r.a.w, &r.a.p, r.a.device, &bctx) != CMGPU_OK) die(cmgpu_last_error(nullptr));
  ck(bctx, cmgpu_save_index_file(bctx, r.a.out_path.c_str()));
  int32_t k, w; uint32_t nb, nocc; uint64_t nmm, nkeys;
  cmgpu_index_info(bctx, &k, &w, &nb, &nocc, &nmm, &nkeys);
  fprintf(stderr, "Collected %llu minimizers.\nLookup table size: %llu, # buckets: %u, occurrence table size: %u.\n",
          (unsigned long long)nmm, (unsigned long long)nkeys, nb, nocc);
  cmgpu_destroy(bctx);
  cmgpu_free_host_ref(&r.ref);
  return 0;
}
static void create_contexts(Run &r, Warm &warm) {
  const Args &a = r.a;
  cmgpu_index_view idx;
  if (cmgpu_load_index_file(a.index_path.c_str(), &idx) != 0) die("Cannot read index " + a.index_path);
  fprintf(stderr, "Kmer size: %d, window size: %d.\n", idx.kmer_size, idx.window_size);
  r.ctxs.assign((size_t)a.gpus, nullptr);
  warm.join();
  if (!warm.out_opened) die("cannot write " + a.out_path);
  for (int gi = 0; gi < a.gpus; ++gi)
    if (cmgpu_create(&idx, &r.ref, &a.p, a.device + gi, &r.ctxs[gi]) != CMGPU_OK) die(cmgpu_last_error(nullptr));
  cmgpu_free_host_index(&idx);
}

// ranks of `names` under an order file (Chromap::GenerateCustomRidRanks, chromap.cc:867-913): ranks from the listed names, unlisted
// sequences follow in reference order
static std::vector<uint32_t> ranks_from_file(const std::string &path, const std::vector<const char *> &names) {
  FILE *of = fopen(path.c_str(), "r");
  if (!of) die("Cannot open chromosome order file " + path);
  std::vector<std::string> order;
  char lb[4096];
  while (fgets(lb, sizeof(lb), of)) { size_t l = strlen(lb); while (l && (lb[l - 1] == '\n' || lb[l - 1] == '\r')) lb[--l] = 0; order.push_back(lb); }
  fclose(of);
  std::vector<uint32_t> rank(names.size(), 0xffffffffu);
  // later lines win for a repeated name, like the reference's map assignment
  for (size_t i = 0; i < names.size(); ++i)
    for (size_t j = 0; j < order.size(); ++j) if (order[j] == names[i]) rank[i] = (uint32_t)j;
  std::vector<std::string> uniq(order);
  std::sort(uniq.begin(), uniq.end());
  uint32_t k = (uint32_t)(std::unique(uniq.begin(), uniq.end()) - uniq.begin());  // distinct names = first free rank
  for (size_t i = 0; i < names.size(); ++i) if (rank[i] == 0xffffffffu) rank[i] = k++;
  if (k > names.size()) die("ERROR: unknown chromsome names found in chromosome order file.");
  return rank;
}
// --chr-order: names / lengths for the writers are permuted like the ranks; --pairs-natural-chr-order: ranks over the (possibly
// reordered) sequences, like the reference computes it
static void apply_chr_orders(Run &r) {
  const cmgpu_ref_view &ref = r.ref;
  r.out_names.assign(ref.names, ref.names + ref.n_sequences);
  r.out_lengths.assign(ref.lengths, ref.lengths + ref.n_sequences);
  if (!r.a.chr_order_path.empty()) {
    const std::vector<uint32_t> rank = ranks_from_file(r.a.chr_order_path, r.out_names);
    for (cmgpu_ctx *cx : r.ctxs) ck(cx, cmgpu_set_chr_order(cx, rank.data(), ref.n_sequences));
    for (uint32_t i = 0; i < ref.n_sequences; ++i) { r.out_names[rank[i]] = ref.names[i]; r.out_lengths[rank[i]] = ref.lengths[i]; }
  }
  if (!r.a.pairs_order_path.empty() && r.a.out_pairs) {
    r.pairs_rank = ranks_from_file(r.a.pairs_order_path, r.out_names);
    ck(r.ctx(), cmgpu_set_pairs_chr_order(r.ctx(), r.pairs_rank.data(), ref.n_sequences));
  }
}

// Pairs output (--preset hic, --pairs) goes through the device ingest like BED: stream 0 keeps the read names in HBM and the final
// step renders the text from them (cmgpu_store_format_pairs_resident).  --SAM does too: the streams of read 1 and read 2 keep whole
// reads (names, bases, qualities) in HBM, every batch's alignment records join the SAM record store, and the final step sorts,
// de-duplicates and renders the lines there (cmgpu_store_format_sam; --BAM: BAM records, cmgpu_store_format_bam).  --barcode-translate with --SAM stays on the host parser and
// writer: its CB value needs the table.  --gpus N > 1 with pairs or SAM output is refused by validate().  --host-ingest forces the
// kseq-style parser (the fallback the CMGPU_EFORMAT message names).
static void configure_contexts(Run &r) {
  const Args &a = r.a;
  for (cmgpu_ctx *cx : r.ctxs) {
    if (a.skip_bc_check) cmgpu_set_barcode_check(cx, 0);
    for (int m = 0; m < 3; ++m)
      if (!a.fmt[m].identity() &&
          cmgpu_fastq_set_format(cx, m, (int)a.fmt[m].starts.size(), a.fmt[m].starts.data(), a.fmt[m].ends.data(), a.fmt[m].strand) != CMGPU_OK)
        die("bad --read-format");
  }
  // records travel to the contexts that own their chromosomes (RCCL over xGMI, issued by the library)
  if (r.exchange) ck(r.ctx(), cmgpu_exchange_init_all(r.ctxs.data(), a.gpus));
  // every stream of every context reads what kseq reads -- wrapped lines, FASTA, stray blank lines (CMGPU_FASTX_FREE; plain four-line
  // text stays on the four-line path, cm_ingest.hip)
  if (r.device_ingest)
    for (cmgpu_ctx *cx : r.ctxs)
      for (int m = 0; m < 3; ++m) ck(cx, cmgpu_fastq_set_layout(cx, m, CMGPU_FASTX_FREE));
  if (r.device_ingest && a.out_pairs) ck(r.ctx(), cmgpu_fastq_keep_names(r.ctx(), 0, 1));
  if (r.sam_device) ck(r.ctx(), cmgpu_fastq_keep_reads(r.ctx(), 1));
  if (r.barcoded && a.whitelist.empty()) {  // no whitelist: every barcode is kept as read (chromap.h:897-903); only its length is needed
    FastxReader pk;
    if (!pk.open(a.bc[0])) die("Cannot find sequence file " + a.bc[0]);
    std::string nm, sq, ql;
    if (!pk.record(nm, sq, ql)) die("empty barcode file");
    pk.close();
    a.fmt[2].apply(sq, ql);
    r.bc_len = (uint32_t)sq.size();
  }
}
// --summary: the reads are counted per barcode as each batch is mapped and the duplicate runs where the device resolves them.  SAM
// text written by the host writer (--host-ingest, --barcode-translate) has its duplicates resolved on the host: the writer counts
// those runs (cmgpu_host_summary_begin / _end).  Called after the whitelist is in place: it sizes the table
static void enable_summary(Run &r) {
  if (r.a.summary_path.empty()) return;
  for (cmgpu_ctx *cx : r.ctxs) ck(cx, cmgpu_summary_enable(cx, 1));
  fprintf(stderr, "Summary: cachehit, fric, estfrip and numcacheslots are not computed (written as 0).\n");
}

// the whitelist for barcodes of r.bc_len letters, from its file to the first context; returns the number of barcodes
static uint32_t load_and_set_whitelist(Run &r) {
  uint64_t *keys = nullptr;
  uint32_t nk = 0;
  if (cmgpu_load_whitelist_file(r.a.whitelist.c_str(), r.bc_len, &keys, &nk) != 0) die("ERROR: whitelist and input barcode lengths are not equal!");
  ck(r.ctx(), cmgpu_set_whitelist(r.ctx(), keys, nk, r.bc_len));
  free(keys);
  return nk;
}
// a failed scan: damage the reference would report as such (kseq's -2 for a truncated quality; a bad BGZF block, which only a scan of
// blocks inflated on the device can meet), text the device parser refuses, anything else
static void classify_scan_error(int rc, const std::string &message, bool on_device) {
  if (rc == CMGPU_OK) return;
  if (rc == CMGPU_EFORMAT && ((on_device && strstr(message.c_str(), "BGZF")) || strstr(message.c_str(), "truncated quality"))) die_corrupt(message);
  if (rc == CMGPU_EFORMAT) die(message + " -- rerun with --host-ingest");
  die(message);
}
// whitelist + abundance pre-pass (chromap.h:750-761), barcode files streamed through the device
static void whitelist_prepass_device(Run &r) {
  if (!r.whitelisted()) return;
  const Args &a = r.a;
  cmgpu_ctx *ctx = r.ctx();
  int done = 0;
  uint64_t ns = 0;
  uint32_t nk = 0;
  for (size_t bi = 0; bi < a.bc.size() && !done; ++bi) {  // every barcode file in turn, batches restart per file (chromap.cc:495-543)
    ChunkReader br;
    if (!br.open(a.bc[bi])) die("Cannot find sequence file " + a.bc[bi]);
    size_t target = a.chunk_bytes;
    while (!done) {
      br.fill(target);
      if (br.len == 0) break;
      if (r.bc_len == 0) {  // length of the first barcode: second line of the file
        const char *p = (const char *)memchr(br.text(), '\n', br.len);
        const char *q = p ? (const char *)memchr(p + 1, '\n', br.len - (size_t)(p + 1 - br.text())) : nullptr;
        if (!p || !q) die("barcode file is not FASTQ");
        r.bc_len = (uint32_t)(q - p - 1);
        if (r.bc_len && p[r.bc_len] == '\r') --r.bc_len;
        r.bc_len = a.fmt[2].eff_len(r.bc_len);
        nk = load_and_set_whitelist(r);
      }
      uint32_t cnt = 0;
      const int brc = cmgpu_fastq_scan(ctx, 2, br.text(), br.len, br.eof, &cnt);
      classify_scan_error(brc, cmgpu_last_error(ctx), false);
      uint32_t n = cnt;
      if (!br.eof) n -= n % 500000;
      if (n == 0 && !br.eof) { target *= 2; continue; }
      uint64_t used = 0;
      ck(ctx, cmgpu_fastq_take(ctx, 2, n, &used));
      br.consume((size_t)used);
      ck(ctx, cmgpu_barcode_abundance_resident(ctx, &ns, &done));
      if (br.eof && n == cnt) break;
    }
    br.close();
  }
  fprintf(stderr, "Loaded %u barcodes.\nCompute barcode abundance using %llu.\n", nk, (unsigned long long)ns);
  for (size_t gi = 1; gi < r.ctxs.size(); ++gi) ck(ctx, cmgpu_copy_whitelist(r.ctxs[gi], ctx));
}
// the same over whole barcode files read by the host parser
static void whitelist_prepass_host(Run &r) {
  if (!r.whitelisted()) return;
  const Args &a = r.a;
  uint32_t nk = 0;
  uint64_t ns = 0;
  for (size_t bi = 0; bi < a.bc.size() && ns < 20000000ull; ++bi) {  // batches restart per file (chromap.cc:495-543)
    FastxReader br;
    if (!br.open(a.bc[bi])) die("Cannot find sequence file " + a.bc[bi]);
    std::string nm, sq, ql;
    std::vector<char> bb;
    std::vector<uint32_t> bo(1, 0);
    while (br.record(nm, sq, ql)) { a.fmt[2].apply(sq, ql); bb.insert(bb.end(), sq.begin(), sq.end()); bo.push_back((uint32_t)bb.size()); }
    br.close();
    if (bo.size() < 2) { if (bi == 0) die("empty barcode file"); continue; }
    if (bi == 0) {
      r.bc_len = bo[1] - bo[0];
      nk = load_and_set_whitelist(r);
    }
    ck(r.ctx(), cmgpu_compute_barcode_abundance(r.ctx(), bb.data(), bo.data(), (uint32_t)bo.size() - 1, &ns));
  }
  fprintf(stderr, "Loaded %u barcodes.\nCompute barcode abundance using %llu.\n", nk, (unsigned long long)ns);
}

// ---- the device ingest: FASTQ text goes to the GPU in chunks; lines, records and the SoA batch are built there.
// Batches are dealt to the contexts in turn; a context maps its batch on its own host thread while the next batch is read and parsed
// for the next context.  With more than one context a round ends with the record exchange (collective: every context takes part, with
// an empty batch when the input ran out).
struct Dealer {
  size_t NG, turn = 0;
  std::vector<std::thread> workers;
  std::vector<char> busy;
  std::vector<int> wrc;
  std::vector<cmgpu_stats> wst;
  bool store_sized = false, overlap1;
  uint64_t names_seen = 0, name_bytes_seen = 0, reads_seen[2] = {0, 0};
  explicit Dealer(const Run &r) : NG(r.ctxs.size()), workers(NG), busy(NG, 0), wrc(NG, CMGPU_OK), wst(NG) {
    for (cmgpu_stats &x : wst) memset(&x, 0, sizeof(x));
    overlap1 = NG == 1 && !r.exchange && !getenv("CM_CLI_NO_OVERLAP");  // (the variable: the serial order, for measurements)
  }
};
// the files of one input set, read side by side: read 1, [read 2], [barcodes]
struct Streams {
  ChunkReader rd[3];
  int n = 0, sid[3] = {0, 0, 2};  // sid: the library's stream of each file
  size_t target = 0;
};
static void finish_round(Run &r, Dealer &d) {
  for (size_t gi = 0; gi < d.NG; ++gi) if (d.busy[gi]) { d.workers[gi].join(); d.busy[gi] = 0; }
  for (size_t gi = 0; gi < d.NG; ++gi) ck(r.ctxs[gi], d.wrc[gi]);
  if (r.exchange) {
    run_side_by_side((int)d.NG, false, [&](int gi) { d.wrc[gi] = cmgpu_exchange_step(r.ctxs[gi], nullptr, nullptr); });
    for (size_t gi = 0; gi < d.NG; ++gi) ck(r.ctxs[gi], d.wrc[gi]);
  }
  d.turn = 0;
}
// one reader thread per file: gzip inflation of read 1 / read 2 / barcodes runs side by side
static void fill_streams(const Run &r, Streams &s) {
  // (blocks inflated on the device: a scan per batch, not per chunk -- the first pass of the inflate takes the same time for
  //  a few hundred blocks as for tens of thousands)
  // (... sized to the batch: what a take leaves over is copied and scanned again with the next piece, so a piece far larger than
  //  a batch -- 1 GiB against the ~125 MB of a 500 000-pair batch -- would be re-scanned many times)
  const size_t piece = std::min<size_t>((size_t)1 << 30, std::max<size_t>((size_t)64 << 20, (size_t)r.a.batch_pairs * 256));
  // (a file's FIRST piece is half that: the device starts on it while the rest of a small file -- or the next piece of a large
  //  one -- is still being read; 8 M pairs in two 185 MB files: 30 ms of reading in front of everything else became 17)
  static const size_t first_div = getenv("CM_FIRST_PIECE_DIV") ? (size_t)std::max(1, atoi(getenv("CM_FIRST_PIECE_DIV"))) : 2;
  run_side_by_side(s.n, true, [&](int m) {
    ChunkReader &rd = s.rd[m];
    size_t want = s.target;
    if (rd.on_device() && !r.a.chunk_given && s.target < piece) want = rd.fed == 0 && rd.zready == 0 ? std::max(s.target, piece / first_div) : piece;
    rd.fill(want);
  });
}
// the files' scans (upload, inflate, line index, record checks) run side by side: a host thread and a HIP stream per file.
// cnt[m]: whole records of file m now on the device; returns whether every file has handed over its last bytes
static bool scan_streams(Streams &s, cmgpu_ctx *cx, uint32_t cnt[3]) {
  int src[3] = {CMGPU_OK, CMGPU_OK, CMGPU_OK};
  std::string serr[3];  // a failed scan's own message (two files may fail differently at the same time)
  run_side_by_side(s.n, true, [&](int m) {
    ChunkReader &rd = s.rd[m];
    src[m] = rd.on_device() ? cmgpu_fastq_scan_bgzf(cx, s.sid[m], rd.zdata(), rd.zready, rd.final(), &cnt[m])
                            : cmgpu_fastq_scan(cx, s.sid[m], rd.text(), rd.len, rd.eof, &cnt[m]);
    if (src[m] != CMGPU_OK) serr[m] = cmgpu_last_error_thread();
  });
  bool all_final = true;
  for (int m = 0; m < s.n; ++m) {
    all_final = all_final && s.rd[m].final();
    classify_scan_error(src[m], serr[m], s.rd[m].on_device());
  }
  return all_final;
}
// the input ran out: every file must have done so at the same record, with nothing but blanks behind it
static void check_streams_ended(Streams &s, cmgpu_ctx *cx, const uint32_t cnt[3]) {
  for (int m = 0; m < s.n; ++m)
    if (cnt[m] != 0) die("Numbers of reads and barcodes don't match!");
  // (text inflated on the device: what is left of it must be blank, as only_whitespace() checks for text held here)
  for (int m = 0; m < s.n; ++m)
    if (s.rd[m].on_device()) {
      uint64_t used = 0;
      if (cmgpu_fastq_take(cx, s.sid[m], 0, &used) != CMGPU_OK) die_corrupt(cmgpu_last_error(cx));
    }
}
// n records of every file become the context's next batch.  Returns when the wait for the batch before began and ended
struct Span { double from, to; };
static Span take_and_commit(Run &r, Dealer &d, Streams &s, cmgpu_ctx *cx, uint32_t n, uint32_t scanned) {
  const Args &a = r.a;
  for (int m = 0; m < s.n; ++m) {
    uint64_t used = 0;
    const int trc = cmgpu_fastq_take(cx, s.sid[m], n, &used);
    if (trc == CMGPU_EFORMAT && s.rd[m].on_device()) die_corrupt(cmgpu_last_error(cx));  // (text behind the file's last whole record)
    ck(cx, trc);
    s.rd[m].consume((size_t)used);
  }
  // (one context: its last batch was being mapped under this batch's read, scan and take -- the take gathers into staging buffers
  //  that the commit swaps in, cm_ingest.hip; with several contexts the round's join does the same job)
  const double tj0 = now_s();
  if (d.overlap1 && d.busy[0]) {
    d.workers[0].join();
    d.busy[0] = 0;
    ck(r.ctxs[0], d.wrc[0]);
  }
  const double tj1 = now_s();
  if (!d.store_sized && d.overlap1 && a.p.max_num_best_mappings == 1 && !a.out_sam) {
    // the record store sized once from what the first piece says about the files (records scanned / share of the file they came
    // from, over all input files): grown on demand it doubles each time with an allocation, a copy and a synchronous free
    d.store_sized = true;
    const double fr = s.rd[0].fraction();
    if (fr > 0 && s.rd[0].fsize) {
      uint64_t all = 0;
      for (const std::string &pth : a.r1) { struct stat sb; if (stat(pth.c_str(), &sb) == 0 && S_ISREG(sb.st_mode)) all += (uint64_t)sb.st_size; }
      const double est = (double)scanned / fr * ((double)all / (double)s.rd[0].fsize);
      if (est < 2.0e9) (void)cmgpu_store_reserve(cx, (uint64_t)(est * 1.01) + 1000000, r.barcoded ? 1 : 0);  // (no room: the store grows as before)
    }
  }
  ck(cx, cmgpu_fastq_commit(cx, n, r.next_read_id, r.paired ? 1 : 0, r.barcoded ? 1 : 0));
  return {tj0, tj1};
}
// CM_CLI_TIMES: what the commit added to the name store (pairs) and to the read store, per mate (SAM)
static void report_stores(const Run &r, Dealer &d, cmgpu_ctx *cx) {
  if (r.a.out_pairs) {
    uint64_t nn = 0, nb = 0;
    ck(cx, cmgpu_names_info(cx, &nn, &nb, nullptr));
    fprintf(stderr, "[times] names %llu %llu\n", (unsigned long long)(nn - d.names_seen), (unsigned long long)(nb - d.name_bytes_seen));
    d.names_seen = nn; d.name_bytes_seen = nb;
  }
  if (r.sam_device)
    for (int m = 0; m < (r.paired ? 2 : 1); ++m) {
      uint64_t nr = 0;
      ck(cx, cmgpu_reads_info(cx, m, &nr, nullptr, nullptr, nullptr));
      fprintf(stderr, "[times] reads %d %llu\n", m + 1, (unsigned long long)(nr - d.reads_seen[m]));
      d.reads_seen[m] = nr;
    }
}
// the context's worker thread maps the committed batch and appends its records to the store
static void launch_map(Run &r, Dealer &d, cmgpu_ctx *cx) {
  const size_t gi = d.turn;
  d.workers[gi] = std::thread([&r, &d, gi, cx]() {
    uint64_t k = 0;
    const double tm0 = now_s();
    int rc = cmgpu_map_resident(cx, &k, &d.wst[gi]);
    const double tm1 = now_s();
    if (rc == CMGPU_OK && !r.exchange) rc = r.a.out_sam ? cmgpu_sam_store_append_resident(cx, nullptr) : cmgpu_store_append_resident(cx, nullptr);
    if (r.times) fprintf(stderr, "[times] map %.4f store_append %.4f\n", tm1 - tm0, now_s() - tm1);
    d.wrc[gi] = rc;
  });
  d.busy[gi] = 1;
}
// input set fi, batch by batch
static void map_one_file_set(Run &r, Dealer &d, size_t fi) {
  const Args &a = r.a;
  Streams s;
  s.n = 1 + (r.paired ? 1 : 0) + (r.barcoded ? 1 : 0);
  s.sid[1] = r.paired ? 1 : 2;
  const int team = (int)std::max(2u, std::min(32u, cpu_budget() / (unsigned)s.n));
  for (ChunkReader &x : s.rd) { x.team = team; x.files_side_by_side = s.n; x.dev_inflate = d.NG == 1; }  // (several GPUs take turns: the text cannot stay on one)
  if (!s.rd[0].open(a.r1[fi])) die("Cannot find sequence file " + a.r1[fi]);
  if (r.paired && !s.rd[1].open(a.r2[fi])) die("Cannot find sequence file " + a.r2[fi]);
  if (r.barcoded && !s.rd[s.n - 1].open(a.bc[fi])) die("Cannot find sequence file " + a.bc[fi]);
  s.target = a.chunk_bytes;
  for (;;) {
    uint32_t cnt[3] = {0, 0, 0};
    double t0 = now_s();
    fill_streams(r, s);
    r.t_read += now_s() - t0;
    t0 = now_s();
    cmgpu_ctx *cx = r.ctxs[d.turn];
    const bool all_final = scan_streams(s, cx, cnt);
    const double ts1 = now_s();
    if (r.times)  // which path each scan took: the four-line one, or the general one of layout CMGPU_FASTX_FREE
      for (int m = 0; m < s.n; ++m) {
        int general = 0;
        ck(cx, cmgpu_fastq_scan_info(cx, s.sid[m], &general, nullptr));
        fprintf(stderr, "[times] layout %d %s\n", s.sid[m], general ? "free" : "strict");
      }
    uint32_t n = cnt[0];
    for (int m = 1; m < s.n; ++m) n = cnt[m] < n ? cnt[m] : n;
    if (n > a.batch_pairs) n = a.batch_pairs;
    if (!all_final || n == a.batch_pairs) n -= n % 500000;  // whole reference batches except at the very end
    if (n == 0) {
      if (!all_final) { s.target *= 2; continue; }
      check_streams_ended(s, cx, cnt);
      break;
    }
    const Span wait = take_and_commit(r, d, s, cx, n, cnt[0]);
    r.t_parse += now_s() - t0 - (wait.to - wait.from);
    r.t_map += wait.to - wait.from;
    if (r.times) {
      fprintf(stderr, "[times] scan %.4f take %.4f wait for the batch before %.4f\n", ts1 - t0, wait.from - ts1, wait.to - wait.from);
      report_stores(r, d, cx);
    }
    t0 = now_s();
    launch_map(r, d, cx);
    if (!d.overlap1 && ++d.turn == d.NG) finish_round(r, d);
    r.t_map += now_s() - t0;
    r.num_reads += r.paired ? 2ull * n : n;
    r.next_read_id += n;
    fprintf(stderr, "Mapped %u read%s.\n", n, r.paired ? " pairs" : "s");
  }
  for (int m = 0; m < s.n; ++m) {
    if (!s.rd[m].only_whitespace()) die(kCorrupt);
    s.rd[m].close();
  }
}
static void map_device_ingest(Run &r) {
  Dealer d(r);
  for (size_t fi = 0; fi < r.a.r1.size(); ++fi) map_one_file_set(r, d, fi);
  const double t0 = now_s();
  if (d.turn > 0 || r.exchange || d.busy[0]) finish_round(r, d);  // the last, partial round (empty batches for the contexts beyond it)
  r.t_map += now_s() - t0;
  for (const cmgpu_stats &x : d.wst) {
    r.st.num_candidates += x.num_candidates; r.st.num_mappings += x.num_mappings; r.st.num_mapped_reads += x.num_mapped_reads;
    r.st.num_uniquely_mapped_reads += x.num_uniquely_mapped_reads; r.st.num_barcode_in_whitelist += x.num_barcode_in_whitelist;
    r.st.num_corrected_barcode += x.num_corrected_barcode;
  }
}

// ---- the host parser (--host-ingest; --SAM with --barcode-translate): records read kseq-style, batches uploaded from host arrays
static void map_host_ingest(Run &r) {
  const Args &a = r.a;
  const bool paired = r.paired, barcoded = r.barcoded;
  cmgpu_ctx *ctx = r.ctx();
  HostSam &sam = r.sam;
  for (size_t fi = 0; fi < a.r1.size(); ++fi) {
    FastxReader f1, f2, fb;
    if (!f1.open(a.r1[fi])) die("Cannot find sequence file " + a.r1[fi]);
    if (paired && !f2.open(a.r2[fi])) die("Cannot find sequence file " + a.r2[fi]);
    if (barcoded && !fb.open(a.bc[fi])) die("Cannot find sequence file " + a.bc[fi]);
    bool more = true;
    while (more) {
      std::vector<char> b1, b2, bb, bq;
      std::vector<uint32_t> o1(1, 0), o2(1, 0), bo(1, 0);
      std::string n1, s1, q1, n2, s2, q2, nb, sb, qb;
      uint32_t n = 0;
      while (n < a.batch_pairs) {
        const bool g1 = f1.record(n1, s1, q1);
        const bool g2 = paired ? f2.record(n2, s2, q2) : g1;
        const bool gb = barcoded ? fb.record(nb, sb, qb) : g1;
        if (!g1 && !g2 && !gb) { more = false; break; }
        if (!(g1 && g2 && gb)) die("Numbers of reads and barcodes don't match!");
        a.fmt[0].apply(s1, q1);
        if (paired) a.fmt[1].apply(s2, q2);
        if (barcoded) a.fmt[2].apply(sb, qb);
        b1.insert(b1.end(), s1.begin(), s1.end()); o1.push_back((uint32_t)b1.size());
        if (paired) { b2.insert(b2.end(), s2.begin(), s2.end()); o2.push_back((uint32_t)b2.size()); }
        if (barcoded) { bb.insert(bb.end(), sb.begin(), sb.end()); bq.insert(bq.end(), qb.begin(), qb.end()); bq.resize(bb.size(), 'I'); bo.push_back((uint32_t)bb.size()); }
        if (a.out_pairs) r.read_names.push_back(n1);
        if (a.out_sam) {
          q1.resize(s1.size(), 'I');
          sam.names1.push_back(n1); sam.b1.insert(sam.b1.end(), s1.begin(), s1.end()); sam.q1.insert(sam.q1.end(), q1.begin(), q1.end());
          if (sam.b1.size() > 0xfffffff0ull) die("--SAM holds all reads of a run in host memory with 32-bit offsets: input too large");
          sam.o1.push_back((uint32_t)sam.b1.size());
          if (paired) {
            q2.resize(s2.size(), 'I');
            sam.names2.push_back(n2); sam.b2.insert(sam.b2.end(), s2.begin(), s2.end()); sam.q2.insert(sam.q2.end(), q2.begin(), q2.end());
            if (sam.b2.size() > 0xfffffff0ull) die("--SAM holds all reads of a run in host memory with 32-bit offsets: input too large");
            sam.o2.push_back((uint32_t)sam.b2.size());
          }
        }
        ++n;
      }
      if (n == 0) break;
      r.num_reads += paired ? 2ull * n : n;
      uint64_t k = 0;
      int rc;
      cmgpu_single_batch single{n, r.next_read_id, b1.data(), o1.data()};
      cmgpu_batch pairs{n, r.next_read_id, b1.data(), o1.data(), b2.data(), o2.data()};
      cmgpu_barcode_batch bc{bb.data(), bq.data(), bo.data()};
      if (barcoded) rc = paired ? cmgpu_map_pairs_barcoded(ctx, &pairs, &bc, nullptr, 0, &k, &r.st) : cmgpu_map_single_barcoded(ctx, &single, &bc, nullptr, 0, &k, &r.st);
      else rc = paired ? cmgpu_map_pairs(ctx, &pairs, nullptr, 0, &k, &r.st) : cmgpu_map_single(ctx, &single, nullptr, 0, &k, &r.st);  // (pairs records too)
      ck(ctx, rc);
      if (a.out_sam) {  // alignment records + CIGAR / MD pools of this batch
        uint64_t slots = 0;
        uint32_t cap = 0;
        cmgpu_sam_layout(ctx, &slots, &cap);
        const size_t base = sam.rec.size();
        sam.rec.resize(base + slots);
        sam.cigar.resize((base + slots) * CMGPU_SAM_CIGAR_CAP);
        sam.md_batches.emplace_back((size_t)slots * cap + 1);
        sam.md_caps.push_back(cap);
        sam.batch_slots.push_back(slots);
        ck(ctx, cmgpu_download_sam(ctx, sam.rec.data() + base, sam.cigar.data() + base * CMGPU_SAM_CIGAR_CAP, sam.md_batches.back().data()));
        if (barcoded) {  // CB tag + the barcode's place in the sort key
          const size_t kb = sam.bc.size();
          sam.bc.resize(kb + n);
          ck(ctx, cmgpu_download_barcode_keys(ctx, sam.bc.data() + kb));
        }
      } else {
        // BED and pairs outputs: the records never leave HBM -- they join the device-side store
        ck(ctx, cmgpu_store_append_resident(ctx, nullptr));
      }
      r.next_read_id += n;
      fprintf(stderr, "Mapped %u read%s.\n", n, paired ? " pairs" : "s");
    }
    f1.close(); f2.close(); fb.close();
  }
}
// Chromap::OutputMappingStatistics (chromap.cc:808-823)
static void print_statistics(const Run &r) {
  const cmgpu_stats &st = r.st;
  fprintf(stderr, "Number of reads: %llu.\nNumber of mapped reads: %llu.\nNumber of uniquely mapped reads: %llu.\n"
                  "Number of reads have multi-mappings: %llu.\nNumber of candidates: %llu.\nNumber of mappings: %llu.\n"
                  "Number of uni-mappings: %llu.\nNumber of multi-mappings: %llu.\n",
          (unsigned long long)r.num_reads, (unsigned long long)st.num_mapped_reads, (unsigned long long)st.num_uniquely_mapped_reads,
          (unsigned long long)(st.num_mapped_reads - st.num_uniquely_mapped_reads), (unsigned long long)st.num_candidates,
          (unsigned long long)st.num_mappings, (unsigned long long)st.num_uniquely_mapped_reads,
          (unsigned long long)(st.num_mappings - st.num_uniquely_mapped_reads));
  if (r.whitelisted())
    fprintf(stderr, "Number of barcodes in whitelist: %llu.\nNumber of corrected barcodes: %llu.\n",
            (unsigned long long)st.num_barcode_in_whitelist, (unsigned long long)st.num_corrected_barcode);
}

// the whole (inflated) text of the --barcode-translate file, gzip-compressed or plain
static std::string read_translation_table(const Args &a) {
  std::string table;
  gzFile tf = gzopen(a.translate_path.c_str(), "r");
  if (!tf) die("Cannot open barcode translation file " + a.translate_path);
  char tb[1 << 16];
  for (int got; (got = gzread(tf, tb, sizeof(tb))) > 0;) table.append(tb, (size_t)got);
  gzclose(tf);
  return table;
}
// ---- --output-bgzf: what the plain writers append to the output file goes there as BGZF blocks
// The header lines start the output file: write_to(path) is the library call that writes them.  With --output-bgzf they are rendered
// into a file of their own beside the output, which goes away again, and become stored BGZF blocks: the output never holds plain text.
template <class F>
static void write_header(Run &r, F write_to) {
  const std::string &path = r.a.out_path;
  if (!r.a.output_bgzf) {
    if (write_to(path.c_str()) != CMGPU_OK) die("Cannot write " + path);
    return;
  }
  const std::string tmp = path + ".header.tmp";
  if (write_to(tmp.c_str()) != CMGPU_OK) { remove(tmp.c_str()); die("Cannot write " + tmp); }
  std::string text;
  FILE *f = fopen(tmp.c_str(), "rb");
  if (!f) die("Cannot read " + tmp);
  char buf[1 << 16];
  for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, got);
  fclose(f);
  remove(tmp.c_str());
  if (cmgpu_bgzf_write_host_text(path.c_str(), text.data(), text.size(), 0) != CMGPU_OK) die("Cannot write " + path);
  r.bgzf_text_bytes += text.size();
  r.bgzf_bytes += text.size() + 31 * ((text.size() + 0xff00 - 1) / 0xff00);
}
// a context's text store: plain, or compressed on the device
static void write_section(Run &r, cmgpu_ctx *cx) {
  const char *path = r.a.out_path.c_str();
  if (!r.a.output_bgzf) { ck(cx, cmgpu_store_write_text(cx, path, 1)); return; }
  const double t0 = now_s();
  uint64_t nb = 0, nout = 0, ntext = 0;
  ck(cx, cmgpu_store_compress_text(cx, &nb, &nout));
  r.t_compress += now_s() - t0;
  ck(cx, cmgpu_bgzf_info(cx, nullptr, nullptr, &ntext));
  ck(cx, cmgpu_bgzf_write(cx, path, 1));
  r.bgzf_bytes += nout;
  r.bgzf_text_bytes += ntext;
}
static void bgzf_finish(Run &r) {
  if (!r.a.output_bgzf) return;
  if (cmgpu_bgzf_write_eof(r.a.out_path.c_str()) != CMGPU_OK) die("Cannot write " + r.a.out_path);
  r.bgzf_bytes += 28;
}
// --output-tbi: the tabix index of the section cx compressed last, whose blocks stand at `base` in the output file.  The output is
// complete by now: a text the indexer refuses ends the run with the indexer's words, and without an index file
static void write_tbi(Run &r, cmgpu_ctx *cx, uint64_t base) {
  const std::string path = r.a.out_path + ".tbi";
  const double t0 = now_s();
  uint64_t n = 0;
  const int rc = cmgpu_bgzf_index_tabix(cx, base, &n);
  if (rc != CMGPU_OK) { remove(path.c_str()); ck(cx, rc); }
  ck(cx, cmgpu_tabix_write(cx, path.c_str()));
  fprintf(stderr, "Built the tabix index on the device and wrote %s (%llu bytes before compression) in %.3fs.\n", path.c_str(), (unsigned long long)n, now_s() - t0);
}
// --output-bai: the BAM index of the records cx compressed last, whose blocks stand at `base` in the output file.  The BAM file is
// complete by now and stays: records the indexer refuses end the run with the indexer's words, and without an index file
static void write_bai(Run &r, cmgpu_ctx *cx, uint64_t base) {
  const std::string path = r.a.out_path + ".bai";
  const double t0 = now_s();
  uint64_t n = 0;
  const int rc = cmgpu_bgzf_index_bai(cx, base, r.ref.n_sequences, nullptr, 0, &n);
  if (rc != CMGPU_OK) { remove(path.c_str()); ck(cx, rc); }
  ck(cx, cmgpu_bai_write(cx, path.c_str()));
  fprintf(stderr, "Built the BAM index on the device and wrote %s (%llu bytes) in %.3fs.\n", path.c_str(), (unsigned long long)n, now_s() - t0);
}
// --output-csi: the CSI index of what cx compressed last -- BAM records (bam) or BED / TagAlign lines -- whose blocks stand at `base`
// in the output file.  Depth 5 (ends up to 2^29, as the .tbi / .bai) unless a reference is longer: then 6.  The output file is complete by
// now and stays: what the indexer refuses ends the run with the indexer's words, and without an index file
static void write_csi(Run &r, cmgpu_ctx *cx, uint64_t base, bool bam) {
  const std::string path = r.a.out_path + ".csi";
  const double t0 = now_s();
  uint32_t depth = 5;
  for (uint32_t len : r.out_lengths)
    if (len > (1u << 29)) depth = 6;
  uint64_t n = 0;
  const int rc = bam ? cmgpu_bgzf_index_csi_bam(cx, base, r.ref.n_sequences, nullptr, 0, depth, &n) : cmgpu_bgzf_index_csi_tabix(cx, base, depth, &n);
  if (rc != CMGPU_OK) { remove(path.c_str()); ck(cx, rc); }
  ck(cx, cmgpu_csi_write(cx, path.c_str()));
  fprintf(stderr, "Built the CSI index (depth %u) on the device and wrote %s (%llu bytes before compression) in %.3fs.\n", depth, path.c_str(),
          (unsigned long long)n, now_s() - t0);
}
// ---- the writers: each returns the number of lines written (negative: the file could not be written)
// sort + duplicate removal + MAPQ filter + SAM lines on the device, from the reads and records in HBM
static int64_t write_sam_device(Run &r) {
  cmgpu_ctx *ctx = r.ctx();
  uint64_t nl = 0, nbytes = 0;
  if (r.a.out_bam) {  // --BAM: the same selection, the records and the header in BAM's binary form; both leave as BGZF blocks (parse(): output_bgzf)
    if (r.a.output_bai || r.a.output_csi) ck(ctx, cmgpu_bam_keep_starts(ctx, 1));
    ck(ctx, cmgpu_store_format_bam(ctx, r.out_names.data(), r.out_lengths.data(), r.ref.n_sequences, &r.a.p, r.barcoded ? r.bc_len : 0, &nl, &nbytes));
    write_header(r, [&](const char *path) { return cmgpu_write_bam_header(r.out_names.data(), r.out_lengths.data(), r.ref.n_sequences, path); });
  } else {
    ck(ctx, cmgpu_store_format_sam(ctx, r.out_names.data(), r.out_lengths.data(), r.ref.n_sequences, &r.a.p, r.barcoded ? r.bc_len : 0, &nl, &nbytes));
    write_header(r, [&](const char *path) { return cmgpu_write_sam_header(r.out_names.data(), r.out_lengths.data(), r.ref.n_sequences, path); });
  }
  const uint64_t bai_base = r.bgzf_bytes;  // (the header's blocks)
  write_section(r, ctx);
  bgzf_finish(r);
  if (r.a.output_bai) write_bai(r, ctx, bai_base);
  if (r.a.output_csi) write_csi(r, ctx, bai_base, true);  // (--BAM: validate())
  return (int64_t)nl;
}
// the host writers: sort, duplicate removal and text from the records and reads collected by map_host_ingest
static int64_t write_sam_host(Run &r) {
  const Args &a = r.a;
  const HostSam &s = r.sam;
  if (!a.summary_path.empty()) cmgpu_host_summary_begin();
  uint32_t cap = 1;
  for (uint32_t c : s.md_caps) cap = c > cap ? c : cap;
  std::vector<char> md(s.rec.size() * (size_t)cap + 1);
  size_t slot0 = 0;
  for (size_t b = 0; b < s.md_batches.size(); ++b) {
    for (uint64_t t = 0; t < s.batch_slots[b]; ++t)
      memcpy(md.data() + (slot0 + t) * cap, s.md_batches[b].data() + t * s.md_caps[b], s.md_caps[b]);
    slot0 += s.batch_slots[b];
  }
  std::vector<const char *> n1(s.names1.size()), n2(s.names2.size() ? s.names2.size() : 1, "");
  for (size_t i = 0; i < s.names1.size(); ++i) n1[i] = s.names1[i].c_str();
  for (size_t i = 0; i < s.names2.size(); ++i) n2[i] = s.names2[i].c_str();
  // what the three writers have in common, then each one's own arguments
  auto write = [&](auto writer, auto... own) -> int64_t {
    return writer(r.out_names.data(), r.out_lengths.data(), r.ref.n_sequences, &a.p, s.rec.data(), s.rec.size(), r.paired ? 1 : 0, s.cigar.data(),
                  md.data(), cap, n1.data(), n2.data(), s.b1.data(), s.q1.data(), s.o1.data(),
                  r.paired ? s.b2.data() : nullptr, r.paired ? s.q2.data() : nullptr, r.paired ? s.o2.data() : nullptr, own...);
  };
  if (!r.barcoded) return write(cmgpu_write_sam, a.out_path.c_str());
  if (a.translate_path.empty()) return write(cmgpu_write_sam_barcoded, s.bc.data(), r.bc_len, a.out_path.c_str());
  const std::string table = read_translation_table(a);  // CB:Z: through the translation table
  const int64_t lines = write(cmgpu_write_sam_barcoded_translated, s.bc.data(), r.bc_len, table.data(), (uint64_t)table.size(), a.out_path.c_str());
  if (lines == CMGPU_EFORMAT) die("Barcode does not exist in the translation table.");
  return lines;
}
// sort + MAPQ filter + text on the device; the read names are in HBM already (device ingest) or go up once as a blob (host parser)
static int64_t write_pairs(Run &r) {
  cmgpu_ctx *ctx = r.ctx();
  uint64_t nl = 0, nbytes = 0;
  if (r.device_ingest) {
    ck(ctx, cmgpu_store_format_pairs_resident(ctx, r.out_names.data(), r.ref.n_sequences, &r.a.p, &nl, &nbytes));
  } else {
    std::string blob;
    std::vector<uint64_t> roff(r.read_names.size() + 1, 0);
    for (size_t i = 0; i < r.read_names.size(); ++i) { blob += r.read_names[i]; roff[i + 1] = blob.size(); }
    ck(ctx, cmgpu_store_format_pairs(ctx, r.out_names.data(), r.ref.n_sequences, &r.a.p, blob.data(), roff.data(), (uint32_t)r.read_names.size(), 0, &nl, &nbytes));
  }
  write_header(r, [&](const char *path) {
    return cmgpu_write_pairs_header(r.out_names.data(), r.out_lengths.data(), r.ref.n_sequences, r.pairs_rank.empty() ? nullptr : r.pairs_rank.data(), path);
  });
  write_section(r, ctx);
  bgzf_finish(r);
  return (int64_t)nl;
}
// --barcode-translate for BED (BarcodeTranslator, barcode_translator.h:42-101): the table goes to the first context and is copied to the
// others; every context then renders column 4 of its section through it (cmgpu_store_format)
static void set_translation_tables(Run &r) {
  const std::string table = read_translation_table(r.a);
  const int rc = cmgpu_set_barcode_translation(r.ctx(), table.data(), (uint64_t)table.size());
  if (rc == CMGPU_EINVAL) die("barcode translation file " + r.a.translate_path + " has no line of the form to<TAB or ,>from");
  ck(r.ctx(), rc);
  for (size_t gi = 1; gi < r.ctxs.size(); ++gi) ck(r.ctxs[gi], cmgpu_copy_barcode_translation(r.ctxs[gi], r.ctx()));
}
// BED / TagAlign: sort + duplicate removal + MAPQ filter + Tn5 shift + text, all on the device
static int64_t write_bed(Run &r) {
  const Args &a = r.a;
  const bool paired = r.paired, barcoded = r.barcoded;
  const size_t NG = r.ctxs.size();
  const int kind = a.out_tagalign && paired ? (barcoded ? CMGPU_TEXT_TAGALIGN_PE_BC : CMGPU_TEXT_TAGALIGN_PE)
                   : a.out_tagalign && barcoded ? CMGPU_TEXT_TAGALIGN_SE_BC
                   : barcoded ? (paired ? CMGPU_TEXT_BED_PE_BC : CMGPU_TEXT_BED_SE_BC) : paired ? CMGPU_TEXT_BED_PE : CMGPU_TEXT_BED_SE;
  const double t0 = now_s();
  if (barcoded && !a.translate_path.empty() && (kind == CMGPU_TEXT_BED_PE_BC || kind == CMGPU_TEXT_BED_SE_BC)) set_translation_tables(r);
  // every context sorts, de-duplicates and renders the chromosomes it owns (all of them with one context)
  std::vector<int> rcs(NG, CMGPU_OK);
  std::vector<uint64_t> nls(NG, 0), nbs(NG, 0);
  run_side_by_side((int)NG, false, [&](int gi) {
    rcs[gi] = cmgpu_store_format(r.ctxs[gi], kind, r.out_names.data(), r.ref.n_sequences, &a.p, r.bc_len, &nls[gi], &nbs[gi]);
  });
  uint64_t nl = 0, nbytes = 0;
  for (size_t gi = 0; gi < NG; ++gi) {
    ck(r.ctxs[gi], rcs[gi]);  // (CMGPU_EFORMAT: "Barcode does not exist in the translation table.", the reference's words)
    nl += nls[gi];
    nbytes += nbs[gi];
  }
  const double t1 = now_s();
  if (a.p.allocate_multi_mappings) {
    if (a.p.low_memory_mode) {
      fprintf(stderr, "--allocate-multi-mappings does nothing in low-memory mode (--low-mem, --preset): no multi-mapping is allocated.\n");
    } else {  // MappingProcessor::AllocateMultiMappings' lines (mapping_processor.h:368, 435-439); one context: validate()
      uint64_t n_multi = 0, n_allocated = 0, n_without = 0;
      int64_t us = 0;
      ck(r.ctx(), cmgpu_store_allocation_info(r.ctx(), &n_multi, &n_allocated, &n_without));
      (void)cmgpu_get_option(r.ctx(), "alloc_us", &us);
      fprintf(stderr, "Got all %llu multi-mappings!\nAllocated %llu multi-mappings in %.3fs.\n# multi-mappings that have no uni-mapping overlaps: %llu.\n",
              (unsigned long long)n_multi, (unsigned long long)n_allocated, (double)us * 1e-6, (unsigned long long)n_without);
    }
  }
  // sections in rank order: the owners hold contiguous, increasing chromosome ranges
  const uint64_t tbi_base = r.bgzf_bytes;
  for (cmgpu_ctx *cx : r.ctxs) write_section(r, cx);  // (emptied at the start)
  bgzf_finish(r);
  if (a.output_tbi) write_tbi(r, r.ctx(), tbi_base);  // (one context: validate())
  if (a.output_csi) write_csi(r, r.ctx(), tbi_base, false);
  r.t_post = now_s() - t0;
  fprintf(stderr, "Sorted, deduplicated and formatted %llu bytes on the device in %.3fs, wrote them in %.3fs.\n", (unsigned long long)nbytes,
          t1 - t0, now_s() - t1);
  return (int64_t)nl;
}

// --summary: the contexts' tables (a multi-GPU run: reads were counted where they were mapped, runs where their chromosome is owned) as one CSV
static void write_summary_csv(Run &r) {
  const Args &a = r.a;
  const size_t NG = r.ctxs.size();
  std::vector<std::vector<cmgpu_summary_entry>> ent(NG + 1);
  std::vector<cmgpu_summary_table> tabs(NG);
  for (size_t gi = 0; gi < NG; ++gi) {
    uint64_t nk = 0, got = 0;
    ck(r.ctxs[gi], cmgpu_summary_info(r.ctxs[gi], &nk, nullptr));
    ent[gi].resize(nk + 1);
    ck(r.ctxs[gi], cmgpu_summary_download(r.ctxs[gi], ent[gi].data(), nk, &got, &tabs[gi].nonwhitelist_total));
    tabs[gi].entries = ent[gi].data();
    tabs[gi].n_entries = got;
  }
  if (a.out_sam && !r.sam_device) {  // the runs the host SAM writer resolved
    uint64_t nk = 0;
    int src = cmgpu_host_summary_end(nullptr, 0, &nk);  // (no room: the number of entries; an empty collector is closed by this call)
    ent.back().resize(nk + 1);
    if (src == CMGPU_ECAPACITY) src = cmgpu_host_summary_end(ent.back().data(), nk, &nk);
    if (src != CMGPU_OK) die("summary: the host writer's counts are missing");
    cmgpu_summary_table t;
    t.entries = ent.back().data(); t.n_entries = nk; t.nonwhitelist_total = 0;
    tabs.push_back(t);
  }
  // (single-end runs always have the last column: MapSingleEndReads calls OutputSummaryMetadata with its defaults, chromap.h:630)
  if (cmgpu_write_summary(tabs.data(), (uint32_t)tabs.size(), r.barcoded ? r.bc_len : 0, !a.whitelist.empty() && !a.p.output_mappings_not_in_whitelist,
                          a.out_sam && r.paired, a.summary_cache_slots || !r.paired, a.summary_path.c_str()) != CMGPU_OK)
    die("cannot write " + a.summary_path);
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "--inflate-only")) return inflate_only(argv[2]);
  Run r;
  r.a = parse(argc, argv);
  validate(r.a);
  r.times = getenv("CM_CLI_TIMES") != nullptr;
  setenv("CM_FQ_EARLY", "1", 0);  // (the files' HIP streams are made with the context: on hardware queues of their own, cm_api.hip)
  Warm warm;
  warm.start(r.a);
  if (cmgpu_load_reference_fasta(r.a.ref_path.c_str(), &r.ref) != 0) die("Cannot find sequence file " + r.a.ref_path);
  fprintf(stderr, "Loaded all sequences successfully, number of sequences: %u.\n", r.ref.n_sequences);
  if (r.a.build_index) return build_index(r, warm);
  const Args &a = r.a;
  r.paired = !a.r2.empty();
  r.barcoded = !a.bc.empty();
  r.exchange = a.gpus > 1 || a.force_exchange;
  r.device_ingest = !a.host_ingest && !(a.out_sam && !a.translate_path.empty());
  r.sam_device = a.out_sam && r.device_ingest;
  memset(&r.st, 0, sizeof(r.st));
  create_contexts(r, warm);
  apply_chr_orders(r);
  r.t_begin = now_s();
  configure_contexts(r);
  if (r.device_ingest) {
    whitelist_prepass_device(r);
    enable_summary(r);
    map_device_ingest(r);
  } else {
    whitelist_prepass_host(r);
    enable_summary(r);
    map_host_ingest(r);
  }
  print_statistics(r);
  const int64_t lines = r.sam_device ? write_sam_device(r) : a.out_sam ? write_sam_host(r) : a.out_pairs ? write_pairs(r) : write_bed(r);
  if (lines < 0) die("cannot write " + a.out_path);
  fprintf(stderr, "Number of output mappings (passed filters): %lld\n", (long long)lines);
  if (!a.summary_path.empty()) write_summary_csv(r);
  if (r.device_ingest)
    fprintf(stderr, "Mapped all reads in %.2fs (file read + inflate %.2fs, H2D + device FASTQ parse %.2fs, mapping %.2fs, post-processing + write %.2fs).\n",
            now_s() - r.t_begin, r.t_read, r.t_parse, r.t_map, r.t_post);
  if (a.out_bam)
    fprintf(stderr, "Compressed %llu bytes of BAM header and records into %llu bytes of BGZF on the device in %.3fs.\n", (unsigned long long)r.bgzf_text_bytes,
            (unsigned long long)r.bgzf_bytes, r.t_compress);
  else if (a.output_bgzf)
    fprintf(stderr, "Compressed %llu bytes of text into %llu bytes of BGZF on the device in %.3fs.\n", (unsigned long long)r.bgzf_text_bytes,
            (unsigned long long)r.bgzf_bytes, r.t_compress);
  for (cmgpu_ctx *cx : r.ctxs) cmgpu_destroy(cx);
  cmgpu_free_host_ref(&r.ref);
  return 0;
}
