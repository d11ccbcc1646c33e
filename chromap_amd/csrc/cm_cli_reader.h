// cm_cli_reader.h -- how `chromap-amd` (cm_cli.cpp) gets at the bytes of its input files: a kseq-style record reader for the host parser,
// and the chunk reader that feeds the device ingest (plain text, gzip, BGZF; read-ahead).  No mapping logic and no call into the library.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <zlib.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include "cm_pargz.h"

static unsigned cpu_budget();  // (these three: cm_cli.cpp)
static void die(const std::string &m);
static void die_corrupt(const std::string &detail);

struct FastxReader {
  gzFile f = nullptr;
  std::vector<char> buf;
  bool open(const std::string &path) {
    f = gzopen(path.c_str(), "r");
    if (f) gzbuffer(f, 1 << 20);
    buf.resize(1 << 16);
    return f != nullptr;
  }
  bool line(std::string &out) {
    out.clear();
    for (;;) {
      if (!gzgets(f, buf.data(), (int)buf.size())) return !out.empty();
      size_t l = strlen(buf.data());
      const bool eol = l > 0 && buf[l - 1] == '\n';
      while (l > 0 && (buf[l - 1] == '\n' || buf[l - 1] == '\r')) --l;
      out.append(buf.data(), l);
      if (eol) return true;
    }
  }
  // one FASTQ/FASTA record: name up to the first whitespace, sequence, quality (may be empty)
  std::string pending;
  // like SequenceBatch::LoadOneSequenceAndSaveAt (sequence_batch.cc:22-62): a record with an empty sequence is skipped, per stream
  bool record(std::string &name, std::string &seq, std::string &qual) {
    while (record_any(name, seq, qual))
      if (!seq.empty()) return true;
    return false;
  }
  bool record_any(std::string &name, std::string &seq, std::string &qual) {
    std::string ln;
    for (;;) {
      if (!pending.empty()) { ln.swap(pending); pending.clear(); }
      else if (!line(ln)) return false;
      if (!ln.empty() && (ln[0] == '@' || ln[0] == '>')) break;
    }
    const bool fq = ln[0] == '@';
    size_t e = 1;
    while (e < ln.size() && ln[e] != ' ' && ln[e] != '\t') ++e;
    name.assign(ln, 1, e - 1);
    seq.clear();
    qual.clear();
    std::string s;
    while (line(s)) {
      if (fq && !s.empty() && s[0] == '+') break;
      if (!fq && !s.empty() && s[0] == '>') { pending = s; break; }
      seq += s;
    }
    if (fq) {
      while (qual.size() < seq.size() && line(s)) qual += s;
    }
    return true;
  }
  void close() { if (f) gzclose(f); f = nullptr; }
};

// raw (inflated) file bytes in large chunks for the device-side FASTQ parser.
// bytes grown without zero-filling (the file's bytes overwrite them); reserve keeps the first `keep` bytes
struct RawBuf {
  unsigned char *p = nullptr;
  size_t cap = 0;
  unsigned char *data() { return p; }
  const unsigned char *data() const { return p; }
  const char *text() const { return reinterpret_cast<const char *>(p); }
  void reserve(size_t n, size_t keep) {
    if (n <= cap) return;
    void *qv = nullptr;
    if (posix_memalign(&qv, (size_t)2 << 20, n) != 0 || !qv) die("out of memory (input buffer)");
    (void)madvise(qv, n, MADV_HUGEPAGE);  // (hundreds of MB touched for the first time: 2 MiB pages where the system gives them)
    unsigned char *q = static_cast<unsigned char *>(qv);
    if (keep) memcpy(q, p, keep);
    free(p);
    p = q;
    cap = n;
  }
  RawBuf() = default;
  RawBuf(const RawBuf &) = delete;
  RawBuf &operator=(const RawBuf &) = delete;
  ~RawBuf() { free(p); }
};
// Plain text is read as it is, ordinary gzip goes through zlib's gzread (one inflating thread per file).  BGZF (bgzip; SAM spec 4.1: a
// series of gzip members of at most 64 KiB, each carrying its compressed size in a 'BC' extra field) is not inflated here when one
// GPU maps: the block headers are walked without decoding and whole compressed blocks go to the device (cmgpu_fastq_scan_bgzf).
// With several GPUs taking turns (the text a batch leaves over lives on one of them) it is inflated block-parallel on the host: the
// ISIZE trailers give every block's place in the output, and a team of threads inflates the blocks of a chunk side by side --
// kseq behind one gzread per file (sequence_batch.cc:22-62) caps the reference's ingest at the rate of one
// inflating core.  Except on that host path, the next piece of the file is read (gzip: inflated) by a thread of its own while the
// device works on the one before.
struct ChunkReader {
  gzFile f = nullptr;
  ParGunzip pg;          // ordinary gzip of 16 MiB and more: inflated by several threads (cm_pargz.h); pargz says it is in use
  bool pargz = false;
  FILE *raw = nullptr;   // BGZF and plain text: the file itself
  bool bgzf = false;
  bool plain = false;    // not gzip at all: `raw` is read directly (gzread would copy the bytes twice)
  int team = 4;          // inflating threads for BGZF input
  int files_side_by_side = 1;  // how many files are read at the same time as this one (read 1, read 2, barcodes): the processors are shared
  RawBuf bufs[2];        // the text: bufs[cur][off .. off + len); the other buffer takes the read-ahead (the two swap: their pages stay mapped)
  int cur = 0;
  std::vector<unsigned char> cbuf;
  size_t off = 0, len = 0;
  bool eof = false;
  // read-ahead: while the device parses and maps what fill() returned, a thread reads (plain text), inflates (gzip) or reads the
  // compressed blocks of (BGZF for the device) the next piece behind the bytes in use; the next fill() takes it over
  std::thread ahead;
  bool ahead_on = false, ahead_eof = false;
  size_t ahead_got = 0;
  const char *text() const { return bufs[cur].text() + off; }
  // how much of the file the records handed out so far came from, 0: unknown (a pipe; gzip inflated by several threads).  What a run uses
  // to size its record store once, after the first batch, instead of doubling it as it fills
  uint64_t fsize = 0, fed = 0;  // fed: bytes of the file whose records have been consumed (BGZF for the device: blocks handed over)
  double fraction() const {
    if (!fsize) return 0;
    if (on_device()) return (double)(fed + zready) / (double)fsize;
    if (plain) return (double)fed / (double)fsize;
    if (f && !pargz) { const z_off_t o = gzoffset(f); return o > 0 ? (double)o / (double)fsize : 0; }
    return 0;
  }
  // `want` bytes of the file itself from raw's position, which moves on: large reads of a regular file by four threads (one thread copies
  // out of the page cache at ~5 GB/s: 185 MB of BGZF blocks per file and 4 M-pair batch took as long as the device took to inflate and
  // parse the batch before -- 0.11 s of a 32 M-pair job's 0.51 s waiting for read-ahead).  Returns the bytes read (< want: the file's end)
  size_t read_raw(unsigned char *dst, size_t want) {
    const off_t pos = fsize ? ftello(raw) : (off_t)-1;
    if (pos < 0 || want < ((size_t)32 << 20) || getenv("CM_READ_THREADS_1")) return fread(dst, 1, want, raw);
    const size_t avail = fsize > (uint64_t)pos ? (size_t)(fsize - (uint64_t)pos) : 0;
    const size_t n = want < avail ? want : avail;
    const int fd = fileno(raw);
    const int k = 4;
    const size_t per = ((n / (size_t)k) + 4095) & ~(size_t)4095;
    std::atomic<bool> ok{true};
    std::thread th[4];
    auto part = [&](int i) {
      size_t o = per * (size_t)i;
      const size_t end = i == k - 1 ? n : (o + per < n ? o + per : n);
      while (o < end) {
        const ssize_t r = pread(fd, dst + o, end - o, pos + (off_t)o);
        if (r <= 0) { ok = false; return; }
        o += (size_t)r;
      }
    };
    for (int i = 1; i < k; ++i) th[i] = std::thread(part, i);
    part(0);
    for (int i = 1; i < k; ++i) th[i].join();
    if (!ok) die_corrupt("read error");
    if (fseeko(raw, pos + (off_t)n, SEEK_SET) != 0) die_corrupt("seek error");
    return n;
  }
  // up to `want` bytes of the (inflated) stream: plain text or gzip
  size_t read_some(unsigned char *dst, size_t want, bool *hit_eof) {
    size_t got = 0;
    while (got < want && !*hit_eof) {
      if (plain) {
        const size_t r = read_raw(dst + got, want - got);
        if (r == 0) { if (ferror(raw)) die_corrupt("read error"); *hit_eof = true; }
        got += r;
      } else if (pargz) {
        size_t g = 0;
        bool e = false;
        if (!pg.read(dst + got, want - got, &g, &e)) die_corrupt(pg.error);
        got += g;
        if (e) *hit_eof = true;
      } else {
        const size_t piece = want - got < (1u << 30) ? want - got : (1u << 30);
        const int r = gzread(f, dst + got, (unsigned)piece);
        if (r < 0) { int en = 0; const char *msg = gzerror(f, &en); die_corrupt(msg ? msg : "read error"); }
        if (r == 0) *hit_eof = true; else got += (size_t)r;
      }
    }
    return got;
  }
  void join_ahead() {
    if (!ahead_on) return;
    ahead.join();
    ahead_on = false;
    // (plain text / gzip: fill() joins the two buffers; BGZF for the device: fill_bgzf_compressed does)
  }
  bool open(const std::string &path) {
    off = 0;
    len = 0;
    eof = false;
    bgzf = false;
    plain = false;
    // only a regular file is sniffed for BGZF: the 18 bytes read from a FIFO, a process substitution or /dev/stdin would be
    // lost to the gzopen below (the reference opens every input with one gzopen, which works on pipes)
    struct stat sb;
    if (stat(path.c_str(), &sb) != 0) return false;
    fsize = S_ISREG(sb.st_mode) ? (uint64_t)sb.st_size : 0;
    fed = 0;
    if (!S_ISREG(sb.st_mode)) {
      f = gzopen(path.c_str(), "r");
      if (f) gzbuffer(f, 1 << 20);
      return f != nullptr;
    }
    raw = fopen(path.c_str(), "rb");
    if (!raw) return false;
    unsigned char h[18];
    const size_t got = fread(h, 1, 18, raw);
    if (got == 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4) && h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C' && h[14] == 2 && h[15] == 0) {
      bgzf = true;
      fseek(raw, 0, SEEK_SET);
      return true;
    }
    if (!(got >= 2 && h[0] == 0x1f && h[1] == 0x8b)) {
      plain = true;
      fseek(raw, 0, SEEK_SET);
      return true;
    }
    fclose(raw);
    raw = nullptr;
    // ordinary gzip: several inflating threads for a file of 16 MiB and more (CM_PARGZ=0: always zlib's gzread; CM_PARGZ_THREADS)
    pargz = false;
    const char *off_env = getenv("CM_PARGZ");
    if (!(off_env && off_env[0] == '0')) {
      // a team per file of the budget over the files read side by side.  (Two teams per file work at a time -- one decodes the next group while
      // the other finishes the last -- so this is twice the budget in threads; measured on a 16-CPU quota, two files: teams of 4 / 6 / 8 / 12 /
      // 32: 1.13 / 0.93 / 0.85 / 0.94 / 0.86-1.06 s end to end)
      const unsigned share = cpu_budget() / (unsigned)(files_side_by_side > 0 ? files_side_by_side : 1);
      int nt = (int)(share < 2 ? 2 : (share > 32 ? 32 : share));
      if (getenv("CM_PARGZ_THREADS")) nt = atoi(getenv("CM_PARGZ_THREADS"));
      if (pg.open(path.c_str(), nt)) { pargz = true; return true; }
    }
    f = gzopen(path.c_str(), "r");
    if (f) gzbuffer(f, 1 << 20);
    return f != nullptr;
  }
  // device inflate (one GPU): the blocks stay compressed -- zdata()[0 .. zready) holds whole blocks whose inflated size adds up to at
  // least `target` more text (the device keeps the text itself, cmgpu_fastq_scan_bgzf), zdata()[zready .. zlen) what was read beyond
  // them (the file is read in large pieces); pending: inflated bytes handed over and not yet taken
  bool dev_inflate = false;
  size_t pending = 0, zoff = 0, zlen = 0, zready = 0;  // (zb[zcur][zoff .. zoff + zlen) is in use)
  // two buffers taking turns: the blocks handed over stay where they are while the device inflates them, the read-ahead goes into the OTHER
  // buffer behind a gap, and the next call copies the few bytes left over in front of it.  (One buffer, round 6's first form: room for the
  // read-ahead meant moving the whole piece in use to the buffer's start -- 185 MB per file and batch, 0.11 s of a 32 M-pair job's 0.51 s)
  static constexpr size_t kZGap = (size_t)72 << 20;  // (what a call may leave over: the 64 MiB its last synchronous read took, and a block)
  RawBuf zb[2];
  int zcur = 0;
  const unsigned char *zdata() const { return zb[zcur].data() + zoff; }
  void fill_bgzf_compressed(size_t target) {
    const bool had_ahead = ahead_on;
    if (ahead_on) { ahead.join(); ahead_on = false; }
    fed += zready;
    zoff += zready;  // (handed over by the last call)
    zlen -= zready;
    zready = 0;
    size_t isum = 0;
    auto room = [&](size_t more) {  // the buffer in use takes `more` bytes behind the ones in use
      RawBuf &z = zb[zcur];
      if (zoff + zlen + more <= z.cap) return;
      if (zoff) { memmove(z.data(), z.data() + zoff, zlen); zoff = 0; }
      if (zlen + more > z.cap) z.reserve(zlen + more + (zlen + more) / 2, zlen);
    };
    if (had_ahead) {
      RawBuf &o = zb[1 - zcur];
      if (zlen <= kZGap) {  // what was left over, in front of what was read ahead
        memcpy(o.data() + kZGap - zlen, zb[zcur].data() + zoff, zlen);
        zcur = 1 - zcur;
        zoff = kZGap - zlen;
        zlen += ahead_got;
      } else {  // (more left over than the gap takes: the read-ahead moves behind it)
        room(ahead_got);
        memcpy(zb[zcur].data() + zoff + zlen, o.data() + kZGap, ahead_got);
        zlen += ahead_got;
      }
      if (ahead_eof) eof = true;
    }
    auto need = [&](size_t upto) {  // at least `upto` bytes in use, or the file has no more
      while (zlen < upto && !eof) {
        const size_t want = std::max(upto - zlen, (size_t)64 << 20);
        room(want);
        const size_t got = read_raw(zb[zcur].data() + zoff + zlen, want);
        zlen += got;
        if (got < want) eof = true;
      }
      return zlen >= upto;
    };
    while (pending + isum < target) {
      if (!need(zready + 18)) {
        if (zlen == zready) break;  // the end of the file, at a block's end
        die_corrupt("truncated BGZF block");
      }
      const unsigned char *h = zdata() + zready;
      if (h[0] != 0x1f || h[1] != 0x8b || h[12] != 'B' || h[13] != 'C')
        die_corrupt("not a BGZF block");
      const size_t bsize = ((size_t)h[16] | ((size_t)h[17] << 8)) + 1;
      if (bsize < 26) die_corrupt("BGZF block size");
      if (!need(zready + bsize)) die_corrupt("truncated BGZF block");
      const unsigned char *t = zdata() + zready + bsize - 4;
      isum += (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16) | ((size_t)t[3] << 24);
      zready += bsize;
    }
    pending += isum;
    // (`eof` for the caller: nothing left to hand over after these blocks)
    if (!eof && zlen == zready) {
      const int ch = fgetc(raw);
      if (ch == EOF) eof = true; else ungetc(ch, raw);
    }
    if (!eof) {  // as many bytes again, read while the device works on these -- into the other buffer, with room behind for one more synchronous read
      const size_t want = std::max(zready, (size_t)64 << 20);
      RawBuf &o = zb[1 - zcur];
      o.reserve(kZGap + want + ((size_t)66 << 20), 0);
      unsigned char *dst = o.data() + kZGap;
      ahead_on = true; ahead_got = 0; ahead_eof = false;
      ahead = std::thread([this, dst, want]() { ahead_got = read_raw(dst, want); if (ahead_got < want) ahead_eof = true; });
    }
  }
  bool dev_final() const { return !ahead_on && eof && zlen == zready; }
  bool on_device() const { return bgzf && dev_inflate; }          // this file's blocks are inflated by the device
  bool final() const { return on_device() ? dev_final() : eof; }  // what fill() handed over is the last of the file
  struct Block { size_t coff, csize, isize, ooff; };
  void fill_bgzf(size_t target) {
    while (len < target && !eof) {
      std::vector<Block> blocks;
      size_t csum = 0, isum = 0;
      cbuf.clear();
      while (isum < target - len && blocks.size() < 16384) {
        unsigned char h[18];
        const size_t got = fread(h, 1, 18, raw);
        if (got == 0) { eof = true; break; }
        if (got != 18 || h[0] != 0x1f || h[1] != 0x8b || h[12] != 'B' || h[13] != 'C')
          die_corrupt("not a BGZF block");
        const size_t bsize = ((size_t)h[16] | ((size_t)h[17] << 8)) + 1;  // whole block
        if (bsize < 26) die_corrupt("BGZF block size");
        cbuf.resize(csum + bsize);
        memcpy(cbuf.data() + csum, h, 18);
        if (fread(cbuf.data() + csum + 18, 1, bsize - 18, raw) != bsize - 18)
          die_corrupt("truncated BGZF block");
        const unsigned char *t = cbuf.data() + csum + bsize - 4;
        const size_t isize = (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16) | ((size_t)t[3] << 24);
        blocks.push_back({csum, bsize, isize, isum});
        csum += bsize;
        isum += isize;
      }
      if (blocks.empty()) break;
      bufs[cur].reserve(len + isum, len);  // (off is 0 here)
      const int nt = (int)std::min<size_t>((size_t)team, blocks.size());
      std::vector<std::thread> th;
      std::vector<int> bad((size_t)nt, 0);
      for (int ti = 0; ti < nt; ++ti)
        th.emplace_back([&, ti]() {
          z_stream zs;
          memset(&zs, 0, sizeof(zs));
          if (inflateInit2(&zs, -15) != Z_OK) { bad[ti] = 1; return; }
          for (size_t bi = (size_t)ti; bi < blocks.size(); bi += (size_t)nt) {
            const Block &b = blocks[bi];
            if (b.isize == 0) continue;
            inflateReset(&zs);
            zs.next_in = cbuf.data() + b.coff + 18;
            zs.avail_in = (uInt)(b.csize - 26);
            zs.next_out = bufs[cur].data() + len + b.ooff;
            zs.avail_out = (uInt)b.isize;
            const int rc = inflate(&zs, Z_FINISH);
            if (rc != Z_STREAM_END || zs.avail_out != 0) { bad[ti] = 1; break; }
          }
          inflateEnd(&zs);
        });
      for (std::thread &t : th) t.join();
      for (int x : bad) if (x) die_corrupt("BGZF inflate");
      len += isum;
    }
  }
  static constexpr size_t kGap = (size_t)64 << 20;  // room in front of the read-ahead for what the last batch left over
  void fill(size_t target) {
    if (on_device()) { fill_bgzf_compressed(target); return; }
    if (bgzf) {
      if (off) { memmove(bufs[cur].data(), bufs[cur].data() + off, len); off = 0; }
      bufs[cur].reserve(target, len);
      fill_bgzf(target);
      return;
    }
    if (ahead_on) {
      // what was read ahead sits in the other buffer behind a gap: the bytes still in use go in front of it
      join_ahead();
      RawBuf &o = bufs[1 - cur];
      if (len <= kGap) {
        memcpy(o.data() + kGap - len, bufs[cur].data() + off, len);
        off = kGap - len;
      } else {  // (more left over than the gap takes: the read-ahead moves back)
        o.reserve(len + ahead_got + target, kGap + ahead_got);
        memmove(o.data() + len, o.data() + kGap, ahead_got);
        memcpy(o.data(), bufs[cur].data() + off, len);
        off = 0;
      }
      cur = 1 - cur;
      len += ahead_got;
      if (ahead_eof) eof = true;
    }
    bufs[cur].reserve(off + std::max(len, target), off + len);
    if (len < target && !eof) len += read_some(bufs[cur].data() + off + len, target - len, &eof);
    if (!eof) {
      RawBuf &o = bufs[1 - cur];
      o.reserve(kGap + target, 0);
      unsigned char *dst = o.data() + kGap;
      ahead_on = true; ahead_got = 0; ahead_eof = false;
      ahead = std::thread([this, dst, target]() { ahead_got = read_some(dst, target, &ahead_eof); });
    }
  }
  void consume(size_t used) {
    if (on_device()) { pending -= used < pending ? used : pending; return; }  // (the device keeps the rest)
    off += used;
    len -= used;
    fed += used;
  }
  bool only_whitespace() {
    if (on_device()) return true;  // (what is left on the device at the end holds no record: cmgpu_fastq_scan_bgzf counted none)
    if (ahead_on) fill(1);  // (takes over what was read ahead; nothing more is read: the file has ended)
    for (size_t i = 0; i < len; ++i) { const char ch = text()[i]; if (ch != '\n' && ch != '\r' && ch != ' ' && ch != '\t') return false; }
    return true;
  }
  void close() { if (ahead_on) { ahead.join(); ahead_on = false; } if (f) gzclose(f); f = nullptr; if (raw) fclose(raw); raw = nullptr; if (pargz) { pg.close(); pargz = false; } }
};

// --inflate-only FILE: the ingest reader on its own (tests): inflated bytes of a file to stdout
static int inflate_only(const char *path) {
  ChunkReader rd;
  if (!rd.open(path)) die(std::string("Cannot find sequence file ") + path);
  rd.team = 4;
  for (;;) {
    rd.fill(3u << 20);
    if (rd.len == 0) break;
    const size_t take = rd.eof ? rd.len : rd.len - rd.len / 3;  // leave a tail, like the FASTQ parser does
    fwrite(rd.text(), 1, take, stdout);
    rd.consume(take);
  }
  if (rd.pargz) fprintf(stderr, "pargz chunks=%llu accepted=%llu serial=%llu\n", (unsigned long long)rd.pg.n_spec, (unsigned long long)rd.pg.n_accepted, (unsigned long long)rd.pg.n_serial);
  else fprintf(stderr, "%s\n", rd.bgzf ? "bgzf" : "gzread");
  rd.close();
  return 0;
}
