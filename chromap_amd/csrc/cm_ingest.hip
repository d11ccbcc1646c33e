// cm_ingest.hip -- FASTQ text -> SoA read batch on the device.
// Replaces kseq_read + SequenceBatch::LoadOneSequenceAndSaveAt
// (sequence_batch.cc:22-62, kseq.h): the host only moves (inflated) file bytes; line splitting,
// record validation, the skip of empty sequences (sequence_batch.cc:27-30) and the packing of
// bases / qualities / offsets run as scans and gathers in HBM.
//
//   scan:  16 bytes per thread -> newline counts -> exclusive scan -> newline positions;
//          records = complete groups of four lines; '@' / '+' markers are checked;
//          records with an empty sequence line are dropped from the stream
//   free:  a stream in layout CMGPU_FASTX_FREE whose text fails the four-line check -- wrapped sequence / quality lines, FASTA, stray
//          blank lines -- resolves kseq's record chain over the same line index instead (cm_fastx.h; k_fx_* below): records are then
//          described by their header line, and the take concatenates a record's sequence and quality lines
//   take:  the first n records' sequence (and quality) lines are gathered into the resident
//          batch arrays of that mate; bytes_consumed tells the host where the next chunk starts
//   names: a stream told to keep them (cmgpu_fastq_keep_names) also gathers the taken records' names -- kseq's name.s: the header
//          line after '@' up to the first isspace() byte, ks_getuntil(ks, 0, &seq->name, &c), kseq.h:188 -- into a staging blob;
//          the commit appends them to the context's run-wide name store, which the pairs text is rendered from where it lies
//   reads: with cmgpu_fastq_keep_reads the takes of read 1 and read 2 gather names AND quality lines (at the bases' offsets, --read-format
//          applied as to the bases, reversed for '-'); the commit appends names, bases and qualities to the run-wide read store (per mate,
//          64-bit offsets), which the SAM text is rendered from (cm_sam_post.hip)
#include <hip/hip_runtime.h>
#include <string.h>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "cm_ctx.h"
#include "cm_kernels.h"
#include "cm_inflate.h"
#include "cm_fastx.h"

#define FQ_BLOCK 256
__device__ __forceinline__ uint32_t fq_nl_mask(const uint8_t *__restrict__ text, uint64_t base, uint64_t n) {
  uint32_t m = 0;
  if (base + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4 *>(text + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (((w[k] >> (8 * b)) & 0xff) == '\n') m |= 1u << (4 * k + b);
  } else {
    for (uint32_t i = 0; base + i < n; ++i)
      if (text[base + i] == '\n') m |= 1u << i;
  }
  return m;
}

__global__ __launch_bounds__(FQ_BLOCK) void k_fq_count(const uint8_t *__restrict__ text, uint64_t n, uint32_t n_thr, uint32_t *__restrict__ cnt) {
  const uint32_t t = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (t < n_thr) cnt[t] = __popc(fq_nl_mask(text, (uint64_t)t * 16, n));
}
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_fill(const uint8_t *__restrict__ text, uint64_t n, uint32_t n_thr,
                                                        const uint32_t *__restrict__ off, uint32_t *__restrict__ nl) {
  const uint32_t t = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (t >= n_thr) return;
  uint32_t m = fq_nl_mask(text, (uint64_t)t * 16, n), o = off[t];
  while (m) { const int b = __ffs(m) - 1; nl[o++] = t * 16 + (uint32_t)b; m &= m - 1; }
}

// line L of the chunk: [start, end) without the terminator and without a trailing '\r'
__device__ __forceinline__ void fq_line(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nl, uint32_t line, uint32_t *s, uint32_t *e) {
  const uint32_t st = line == 0 ? 0u : nl[line - 1] + 1u;
  uint32_t en = nl[line];
  if (en > st && text[en - 1] == '\r') --en;
  *s = st;
  *e = en;
}

// per raw record: marker check, sequence length, keep flag (non-empty sequence)
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_records(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nl, uint32_t n_raw,
                                                           int flags, uint32_t *__restrict__ keep, uint32_t *__restrict__ bad) {
  // (bad[0]: first record with a missing marker or -- want_qual -- a quality line of another length than its sequence; bad[1]: first
  //  record whose markers are fine and whose quality line alone is wrong, kseq's "truncated quality")
  // flags: 1 = the quality's length is checked; 2 = layout CMGPU_FASTX_FREE: a sequence line that starts with '@', '+' or '>' is flagged
  // too -- kseq reads such a line as a marker, and the general path (k_fx_*) decides what the text is
  const int want_qual = flags & 1;
  const uint32_t r = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (r >= n_raw) return;
  uint32_t s0, e0, s1, e1, s2, e2, s3, e3;
  fq_line(text, nl, 4 * r, &s0, &e0);
  fq_line(text, nl, 4 * r + 1, &s1, &e1);
  fq_line(text, nl, 4 * r + 2, &s2, &e2);
  fq_line(text, nl, 4 * r + 3, &s3, &e3);
  bool ok = e0 > s0 && text[s0] == '@' && e2 > s2 && text[s2] == '+';
  if ((flags & 2) && e1 > s1) { const uint8_t c1 = text[s1]; if (c1 == '@' || c1 == '+' || c1 == '>') ok = false; }
  // (... and a sequence or quality line that is a lone '\r': kseq keeps that byte, kseq.h:141; fq_line has dropped it, the line's '\n' tells)
  if ((flags & 2) && ((e1 == s1 && nl[4 * r + 1] > s1) || (e3 == s3 && nl[4 * r + 3] > s3))) ok = false;
  if (want_qual && (e3 - s3) != (e1 - s1)) { if (ok) atomicMin(bad + 1, r); ok = false; }  // kseq: quality and sequence lengths must agree
  // a GROUP of four blank lines (spaces and tabs at most) is no record and no damage either -- a file may end in any number of blank
  // lines.  One to three blank lines between two records shift the four-line frame of every record after them: the record is flagged.
  // In layout CMGPU_FASTX_STRICT4 the scan then fails with EFORMAT; in CMGPU_FASTX_FREE the general path reads the chunk as kseq does.
  bool blank = true;
  for (uint32_t i = s0; blank && i < e3; ++i) { const uint8_t ch = text[i]; blank = ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r'; }
  if (!ok && !blank) atomicMin(bad, r);
  keep[r] = !blank && e1 > s1 ? 1u : 0u;
}
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_compact(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos, uint32_t n_raw,
                                                           uint32_t *__restrict__ recidx) {
  const uint32_t r = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (r < n_raw && keep[r]) recidx[pos[r]] = r;
}
// --read-format: which bases of a record are kept (SequenceEffectiveRange::Replace, sequence_effective_range.h:84-122)
struct FqFormat {
  int n_ranges;      // 0: the whole sequence
  int start[4], end[4];
  int minus;         // reverse (and, for bases, complement) after extraction
};
__device__ __forceinline__ uint32_t fq_eff_len(const FqFormat &f, uint32_t len) {
  if (f.n_ranges == 0) return len;
  uint32_t out = 0;
  for (int k = 0; k < f.n_ranges; ++k) {
    int st = f.start[k], en = f.end[k] == -1 ? (int)len - 1 : f.end[k];
    if (en >= (int)len) en = (int)len - 1;  // the reference reads past the end here; ranges are clamped instead
    if (st < 0) st = 0;
    if (en >= st) out += (uint32_t)(en - st + 1);
  }
  return out;
}
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_len(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nl,
                                                       const uint32_t *__restrict__ recidx, uint32_t n, FqFormat fmt, uint32_t *__restrict__ len) {
  const uint32_t j = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (j >= n) return;
  uint32_t s, e;
  fq_line(text, nl, 4 * recidx[j] + 1, &s, &e);
  len[j] = fq_eff_len(fmt, e - s);
}
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_gather(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nl,
                                                          const uint32_t *__restrict__ recidx, const uint32_t *__restrict__ off, uint32_t n,
                                                          FqFormat fmt, uint8_t *__restrict__ bases, uint8_t *__restrict__ quals) {
  const uint32_t j = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (j >= n) return;
  uint32_t s, e, qs = 0, qe = 0;
  fq_line(text, nl, 4 * recidx[j] + 1, &s, &e);
  if (quals) fq_line(text, nl, 4 * recidx[j] + 3, &qs, &qe);
  const uint32_t o = off[j], raw = e - s;
  if (fmt.n_ranges == 0 && !fmt.minus) {
    for (uint32_t i = 0; i < raw; ++i) bases[o + i] = text[s + i];
    if (quals) for (uint32_t i = 0; i < raw; ++i) quals[o + i] = text[qs + i];
    return;
  }
  const uint32_t l = fq_eff_len(fmt, raw);
  uint32_t w = 0;
  const int nr = fmt.n_ranges ? fmt.n_ranges : 1;
  for (int k = 0; k < nr; ++k) {
    int st = fmt.n_ranges ? fmt.start[k] : 0, en = fmt.n_ranges ? (fmt.end[k] == -1 ? (int)raw - 1 : fmt.end[k]) : (int)raw - 1;
    if (en >= (int)raw) en = (int)raw - 1;
    if (st < 0) st = 0;
    for (int p = st; p <= en; ++p, ++w) {
      const uint32_t dst = fmt.minus ? o + (l - 1 - w) : o + w;
      uint8_t c = text[s + (uint32_t)p];
      if (fmt.minus) {  // Uint8ToChar(3 ^ CharToUint8(c))
        const uint8_t u = c & 0xDF;
        c = u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N';
      }
      bases[dst] = c;
      if (quals) quals[dst] = text[qs + (uint32_t)p];
    }
  }
}

// ---- read names ------------------------------------------------------------------------------------------------------------------
// bit 7 of every byte of w for which C's isspace() holds (' ', \t \n \v \f \r); exact per byte: the sums stay below 256, so nothing
// carries from one byte into the next
__device__ __forceinline__ uint64_t fq_space_mask(uint64_t w) {
  const uint64_t L = 0x0101010101010101ull, H = 0x8080808080808080ull;
  const uint64_t x = w & ~H;
  const uint64_t ctl = ~(x + (0x80 - 14) * L) & (x + (0x80 - 9) * L) & ~w;  // 9 <= byte < 14
  const uint64_t y = w ^ (0x20 * L);
  const uint64_t sp = ~(((y & ~H) + ~H) | y);                                // byte == ' '
  return (ctl | sp) & H;
}
// first byte of the name of taken record j: behind the '@' of its header line.  FREE: the record is known by its header line (general path
// of layout CMGPU_FASTX_FREE), not by its place among the groups of four
template <bool FREE>
__device__ __forceinline__ uint32_t fq_name_start(const uint32_t *__restrict__ nl, uint32_t raw) {
  const uint32_t line = FREE ? raw : 4 * raw;
  return (line == 0 ? 0u : nl[line - 1] + 1u) + 1u;
}
// name length of every taken record: the header is read in aligned 16-byte pieces from the piece that holds its first byte on (a
// thread per record: a header is a few tens of bytes, two or three loads).  The line's own '\n' ends the search at the latest; the text
// buffers have 32 bytes of room behind n_bytes, so the last piece stays inside the allocation.
template <bool FREE>
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_name_len(const uint8_t *__restrict__ text, uint64_t n_bytes, const uint32_t *__restrict__ nl,
                                                            const uint32_t *__restrict__ recidx, uint32_t n, uint32_t *__restrict__ len) {
  const uint32_t j = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t s = fq_name_start<FREE>(nl, recidx[j]);
  uint32_t a = s & ~15u, skip = s - a, end = (uint32_t)n_bytes;
  while (a < n_bytes) {
    const uint4 v = *reinterpret_cast<const uint4 *>(text + a);
    uint64_t m0 = fq_space_mask((uint64_t)v.x | ((uint64_t)v.y << 32)), m1 = fq_space_mask((uint64_t)v.z | ((uint64_t)v.w << 32));
    if (skip >= 8) { m0 = 0; m1 &= ~0ull << (8 * (skip - 8)); }  // (bytes of the piece in front of the name)
    else if (skip) m0 &= ~0ull << (8 * skip);
    skip = 0;
    if (m0) { end = a + (uint32_t)(__ffsll((unsigned long long)m0) - 1) / 8u; break; }
    if (m1) { end = a + 8u + (uint32_t)(__ffsll((unsigned long long)m1) - 1) / 8u; break; }
    a += 16u;
  }
  len[j] = end > s ? end - s : 0u;
}
// the names back to back: single bytes up to the destination's next 4-byte boundary, then whole words (the source is read at whatever
// alignment it has), then the last bytes
template <bool FREE>
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_name_gather(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nl,
                                                               const uint32_t *__restrict__ recidx, const uint32_t *__restrict__ off, uint32_t n,
                                                               uint8_t *__restrict__ blob) {
  const uint32_t j = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t o = off[j], len = off[j + 1] - o;
  const uint8_t *src = text + fq_name_start<FREE>(nl, recidx[j]);
  uint8_t *dst = blob + o;
  uint32_t i = 0;
  for (; i < len && ((o + i) & 3u); ++i) dst[i] = src[i];
  for (; i + 4 <= len; i += 4) {
    uint32_t w;
    __builtin_memcpy(&w, src + i, 4);
    *reinterpret_cast<uint32_t *>(dst + i) = w;
  }
  for (; i < len; ++i) dst[i] = src[i];
}
// commit: the batch's n + 1 staging offsets, moved behind the bytes the store already holds, become the store's offsets nm_n .. nm_n + n
__global__ __launch_bounds__(FQ_BLOCK) void k_fq_name_append(const uint32_t *__restrict__ off, uint32_t n, uint64_t base, uint64_t *__restrict__ out) {
  const uint32_t j = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (j <= n) out[j] = base + off[j];
}

// ---- layout CMGPU_FASTX_FREE, general path: kseq's record chain over the line index (cm_fastx.h) -----------------------------------------
__global__ __launch_bounds__(FQ_BLOCK) void k_fx_lines(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nl, uint32_t n_lines,
                                                         uint32_t *__restrict__ li) {
  const uint32_t i = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (i < n_lines) li[i] = cm_fx_line_info(text, nl, i);
}
// a lane per line; only header candidates walk further than their own line, and then the lines of one record
__global__ __launch_bounds__(FQ_BLOCK) void k_fx_walk(const uint32_t *__restrict__ li, uint32_t n_lines, int final_chunk, int unterminated,
                                                        uint32_t *__restrict__ nxt, uint32_t *__restrict__ send, uint32_t *__restrict__ sl) {
  const uint32_t i = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (i >= n_lines) return;
  uint32_t a, b, c;
  cm_fx_walk(li, n_lines, i, final_chunk != 0, unterminated != 0, &a, &b, &c);
  nxt[i] = a; send[i] = b; sl[i] = c;
}
// a block per tile of CM_FX_TILE lines: every line's first chain element behind the tile, by pointer doubling in LDS
__global__ __launch_bounds__(FQ_BLOCK) void k_fx_tile(const uint32_t *__restrict__ nxt, uint32_t n_lines, uint32_t *__restrict__ exit_) {
  __shared__ uint32_t e[CM_FX_TILE];
  const uint32_t t0 = blockIdx.x * CM_FX_TILE, t1 = t0 + CM_FX_TILE < n_lines ? t0 + CM_FX_TILE : n_lines, cnt = t1 - t0;
  for (uint32_t k = threadIdx.x; k < cnt; k += FQ_BLOCK) e[k] = nxt[t0 + k];
  __syncthreads();
  for (int r = 0; r < CM_FX_TILE_ROUNDS; ++r) {
    for (uint32_t k = threadIdx.x; k < cnt; k += FQ_BLOCK) cm_fx_tile_jump(e, t0, t1, k);
    __syncthreads();
  }
  for (uint32_t k = threadIdx.x; k < cnt; k += FQ_BLOCK) exit_[t0 + k] = e[k];
}
// one lane: a step per tile the chain touches (entry: 0xff-filled before)
__global__ void k_fx_entries(const uint32_t *__restrict__ exit_, uint32_t n_lines, uint32_t *__restrict__ entry) {
  if (blockIdx.x == 0 && threadIdx.x == 0) cm_fx_tile_entries(exit_, n_lines, entry);
}
// a lane per tile walks the tile's members: complete records with a sequence are kept (keep: zeroed before), the one member that ends the
// chain early goes to res[0] (line) / res[1] (status), the first record without quality of a stream that needs qualities to res[2], the
// kinds of records kept (CM_FX_SEEN_*) to res[3]
__global__ __launch_bounds__(64) void k_fx_mark(const uint32_t *__restrict__ nxt, const uint32_t *__restrict__ sl, const uint32_t *__restrict__ entry,
                                                uint32_t n_tiles, uint32_t n_lines, int want_qual, uint32_t *__restrict__ keep, uint32_t *__restrict__ res) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_tiles) return;
  const uint32_t first = entry[t];
  if (first == CM_FX_NONE) return;
  const uint32_t t1 = (t + 1) * CM_FX_TILE < n_lines ? (t + 1) * CM_FX_TILE : n_lines;
  uint32_t seen = 0;
  cm_fx_tile_members(nxt, first, t1, [&](uint32_t i) {
    const uint32_t st = sl[i] >> 28, len = sl[i] & CM_FX_LEN_MASK;
    if (st <= CM_FX_FASTA) {
      if (len == 0) return;  // (no record and no name: sequence_batch.cc:27-30)
      if (st == CM_FX_FASTA && want_qual) atomicMin(res + 2, i);
      else { keep[i] = 1u; seen |= st == CM_FX_FASTA ? CM_FX_SEEN_FASTA : CM_FX_SEEN_FASTQ; }
    } else if (st != CM_FX_SKIP) { res[0] = i; res[1] = st; }
  });
  if (seen) atomicOr(res + 3, seen);
}
// the take's kernels for records known by their header line h = recidx[j]: sequence lines (h, send[h]), quality lines (send[h], nxt[h])
__global__ __launch_bounds__(FQ_BLOCK) void k_fx_len(const uint32_t *__restrict__ sl, const uint32_t *__restrict__ recidx, uint32_t n, FqFormat fmt,
                                                       uint32_t *__restrict__ len) {
  const uint32_t j = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (j < n) len[j] = fq_eff_len(fmt, sl[recidx[j]] & CM_FX_LEN_MASK);
}
__global__ __launch_bounds__(FQ_BLOCK) void k_fx_gather(const uint8_t *__restrict__ text, const uint32_t *__restrict__ nl, const uint32_t *__restrict__ nxt,
                                                          const uint32_t *__restrict__ send, const uint32_t *__restrict__ sl,
                                                          const uint32_t *__restrict__ recidx, const uint32_t *__restrict__ off, uint32_t n,
                                                          FqFormat fmt, uint8_t *__restrict__ bases, uint8_t *__restrict__ quals) {
  const uint32_t j = blockIdx.x * FQ_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t h = recidx[j], raw = sl[h] & CM_FX_LEN_MASK, se = send[h], o = off[j], l = off[j + 1] - o;
  cm_fx_copy(text, nl, h + 1, se, raw, fmt.n_ranges, fmt.start, fmt.end, fmt.minus, fmt.minus != 0, o, l, bases);
  if (quals) cm_fx_copy(text, nl, se + 1, nxt[h], raw, fmt.n_ranges, fmt.start, fmt.end, fmt.minus, false, o, l, quals);
}

struct FqMaxOp {
  __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};

// the scan of n_bytes of text resident in f.text (last_char: its last byte): lines, records, markers
static int fq_scan_resident(cmgpu_ctx *c, int stream, uint64_t n_bytes, int final_chunk, char last_char, uint32_t *n_records);
// the HIP stream a FASTQ stream's scan runs on: one each, so that a host thread per file scans read 1, read 2 and the barcodes side by
// side (cmgpu_fastq_scan / _scan_bgzf of DIFFERENT streams of one context may be called concurrently; every call ends synchronised)
static hipStream_t fq_hs(cmgpu_ctx *c, CmFqStream &f) {
  // (made with the context when the process sets CM_FQ_EARLY, cm_api.hip -- on hardware queues of their own; made here, lazily, read 1's
  //  and read 2's streams shared a queue.  A priority of its own for read 2's stream did not separate them: measured, no change)
  if (!f.hs && hipStreamCreateWithFlags(&f.hs, hipStreamNonBlocking) != hipSuccess) { f.hs = nullptr; (void)hipGetLastError(); return c->stream; }
  return f.hs;
}

extern "C" int cmgpu_fastq_scan(cmgpu_ctx *c, int stream, const char *text, uint64_t n_bytes, int final_chunk, uint32_t *n_records) {
  if (!c || stream < 0 || stream > 2 || (!text && n_bytes) || !n_records) return CMGPU_EINVAL;
  if (n_bytes > 0xfffffff0ull) { cm_set_error(c, "FASTQ chunk must be smaller than 4 GiB"); return CMGPU_EINVAL; }
  CM_HIPCHECK(c, cm_enter(c));
  CmFqStream &f = c->fq[stream];
  *n_records = 0;
  f.dev_mode = false; f.dev_len = 0;
  f.n_bytes = n_bytes; f.n_nl = 0; f.n_raw = 0; f.n_rec = 0; f.final_chunk = final_chunk != 0;
  f.general = false; f.fx_lines = 0; f.fx_stop = 0;
  if (n_bytes == 0) return CMGPU_OK;
  if (f.text.ensure(n_bytes + 32)) { cm_set_error(c, "out of device memory (FASTQ text)"); return CMGPU_ENOMEM; }
  CM_HIPCHECK(c, hipMemcpyAsync(f.text.p, text, n_bytes, hipMemcpyHostToDevice, fq_hs(c, f)));
  return fq_scan_resident(c, stream, n_bytes, final_chunk, text[n_bytes - 1], n_records);
}

// layout CMGPU_FASTX_FREE, the chunk is not plain four-line text: the records of its n_lines lines (f.nl) as kseq reads them
static int fq_scan_general(cmgpu_ctx *c, int stream, uint32_t n_lines, bool final_chunk, bool unterminated, uint32_t *n_records) {
  CmFqStream &f = c->fq[stream];
  hipStream_t s = fq_hs(c, f);
  f.general = true;
  f.fx_lines = n_lines; f.fx_stop = 0;
  f.n_raw = 0; f.n_rec = 0;
  *n_records = 0;
  if (n_lines == 0) return CMGPU_OK;
  const uint32_t n_tiles = (n_lines + CM_FX_TILE - 1) / CM_FX_TILE;
  const size_t per_line = ((size_t)n_lines + 1) * 4;
  if (f.fx_li.ensure(per_line) || f.fx_nxt.ensure(per_line) || f.fx_send.ensure(per_line) || f.fx_sl.ensure(per_line) || f.fx_exit.ensure(per_line) ||
      f.fx_entry.ensure((size_t)n_tiles * 4) || f.fx_res.ensure(16) || f.keep.ensure(per_line) || f.pos.ensure(per_line) || f.recidx.ensure(per_line) ||
      f.scan_tmp.ensure(cm_scan_tmp_words(n_lines) * 4)) { cm_set_error(c, "out of device memory (FASTQ records)"); return CMGPU_ENOMEM; }
  const uint32_t none = 0xffffffffu;
  const uint32_t res0[4] = {none, 0u, none, 0u};
  CM_HIPCHECK(c, hipMemcpyAsync(f.fx_res.p, res0, 16, hipMemcpyHostToDevice, s));
  CM_HIPCHECK(c, hipMemsetAsync(f.fx_entry.p, 0xff, (size_t)n_tiles * 4, s));
  CM_HIPCHECK(c, hipMemsetAsync(f.keep.p, 0, per_line, s));
  const dim3 gl((n_lines + FQ_BLOCK - 1) / FQ_BLOCK), b(FQ_BLOCK);
  const int want_qual = stream == 2 || f.keep_reads ? 1 : 0;
  hipLaunchKernelGGL(k_fx_lines, gl, b, 0, s, (const uint8_t *)f.text.p, (const uint32_t *)f.nl.p, n_lines, (uint32_t *)f.fx_li.p);
  hipLaunchKernelGGL(k_fx_walk, gl, b, 0, s, (const uint32_t *)f.fx_li.p, n_lines, final_chunk ? 1 : 0, unterminated ? 1 : 0, (uint32_t *)f.fx_nxt.p,
                     (uint32_t *)f.fx_send.p, (uint32_t *)f.fx_sl.p);
  hipLaunchKernelGGL(k_fx_tile, dim3(n_tiles), b, 0, s, (const uint32_t *)f.fx_nxt.p, n_lines, (uint32_t *)f.fx_exit.p);
  hipLaunchKernelGGL(k_fx_entries, dim3(1), dim3(1), 0, s, (const uint32_t *)f.fx_exit.p, n_lines, (uint32_t *)f.fx_entry.p);
  hipLaunchKernelGGL(k_fx_mark, dim3((n_tiles + 63) / 64), dim3(64), 0, s, (const uint32_t *)f.fx_nxt.p, (const uint32_t *)f.fx_sl.p,
                     (const uint32_t *)f.fx_entry.p, n_tiles, n_lines, want_qual, (uint32_t *)f.keep.p, (uint32_t *)f.fx_res.p);
  cm_scan_u32((const uint32_t *)f.keep.p, (uint32_t *)f.pos.p, n_lines, (uint32_t *)f.scan_tmp.p, s);
  hipLaunchKernelGGL(k_fq_compact, gl, b, 0, s, (const uint32_t *)f.keep.p, (const uint32_t *)f.pos.p, n_lines, (uint32_t *)f.recidx.p);
  uint32_t res[4] = {none, 0, none, 0}, n_rec = 0;
  CM_HIPCHECK(c, hipMemcpyAsync(res, f.fx_res.p, 16, hipMemcpyDeviceToHost, s));
  CM_HIPCHECK(c, hipMemcpyAsync(&n_rec, (uint32_t *)f.pos.p + n_lines, 4, hipMemcpyDeviceToHost, s));
  CM_HIPCHECK(c, cm_stream_sync(s));
  const bool early = res[0] != none, refused = early && res[1] != CM_FX_INCOMPLETE;
  if (res[2] != none && !(refused && res[0] < res[2])) {
    cm_set_error(c, "record without quality (FASTA) at line " + std::to_string(res[2]) + " of the chunk, and " +
                        (stream == 2 ? std::string("the barcode stream needs qualities")
                                     : std::string("whole reads are kept for SAM output (cmgpu_fastq_keep_reads): the reference cannot write SAM for FASTA reads either")));
    return CMGPU_EFORMAT;
  }
  if (refused) {
    const std::string at = " (line " + std::to_string(res[0]) + " of the chunk)";
    if (res[1] == CM_FX_TRUNC) cm_set_error(c, "truncated quality: the quality is not as long as the sequence of the record" + at);
    else if (res[1] == CM_FX_KEPT_CR) cm_set_error(c, "a line that holds only a carriage return starts the sequence or the quality of the record" + at);
    else cm_set_error(c, "neither blank nor a '@' / '>' header where a record is looked for, or a line of 256 MiB and more" + at);
    return CMGPU_EFORMAT;
  }
  f.fx_seen |= res[3];
  if (f.fx_seen == (CM_FX_SEEN_FASTQ | CM_FX_SEEN_FASTA)) {
    cm_set_error(c, "records with quality and records without in one stream: FASTA and FASTQ mixed, or a FASTQ file cut short inside a record (corrupted?)");
    return CMGPU_EFORMAT;
  }
  f.fx_stop = early ? res[0] : n_lines;
  f.n_rec = n_rec;
  *n_records = n_rec;
  return CMGPU_OK;
}

static int fq_scan_resident(cmgpu_ctx *c, int stream, uint64_t n_bytes, int final_chunk, char last_char, uint32_t *n_records) {
  CmFqStream &f = c->fq[stream];
  hipStream_t s = fq_hs(c, f);
  const bool free_layout = f.layout == CMGPU_FASTX_FREE;
  const uint32_t n_thr = (uint32_t)((n_bytes + 15) / 16);
  if (f.cnt.ensure(((size_t)n_thr + 1) * 4) || f.off.ensure(((size_t)n_thr + 1) * 4) ||
      f.scan_tmp.ensure(cm_scan_tmp_words(n_thr) * 4)) { cm_set_error(c, "out of device memory (FASTQ text)"); return CMGPU_ENOMEM; }
  const dim3 g((n_thr + FQ_BLOCK - 1) / FQ_BLOCK), b(FQ_BLOCK);
  hipLaunchKernelGGL(k_fq_count, g, b, 0, s, (const uint8_t *)f.text.p, n_bytes, n_thr, (uint32_t *)f.cnt.p);
  cm_scan_u32((const uint32_t *)f.cnt.p, (uint32_t *)f.off.p, n_thr, (uint32_t *)f.scan_tmp.p, s);
  uint32_t n_nl = 0;
  CM_HIPCHECK(c, hipMemcpyAsync(&n_nl, (uint32_t *)f.off.p + n_thr, 4, hipMemcpyDeviceToHost, s));
  CM_HIPCHECK(c, cm_stream_sync(s));
  if (f.nl.ensure(((size_t)n_nl + 2) * 4)) { cm_set_error(c, "out of device memory (FASTQ lines)"); return CMGPU_ENOMEM; }
  hipLaunchKernelGGL(k_fq_fill, g, b, 0, s, (const uint8_t *)f.text.p, n_bytes, n_thr, (const uint32_t *)f.off.p, (uint32_t *)f.nl.p);
  // a final chunk whose last line has no terminator: the end of the text closes it
  // (also an empty, unterminated quality line of the very last record: three lines seen)
  const bool unterminated = final_chunk && last_char != '\n';
  const uint32_t n_lines = n_nl + (unterminated ? 1u : 0u);  // (the lines of the text; the four-line path below may count an empty one more)
  if (final_chunk && (last_char != '\n' || n_nl % 4 == 3)) {
    const uint32_t endpos = (uint32_t)n_bytes;
    CM_HIPCHECK(c, hipMemcpyAsync((uint32_t *)f.nl.p + n_nl, &endpos, 4, hipMemcpyHostToDevice, s));
    CM_HIPCHECK(c, cm_stream_sync(s));
    ++n_nl;
  }
  f.n_nl = n_nl;
  // (layout FREE: lines behind the last group of four at the end of the text are records or blank lines for the general path to tell)
  if (free_layout && final_chunk && n_lines % 4 != 0) return fq_scan_general(c, stream, n_lines, true, unterminated, n_records);
  const uint32_t n_raw = n_nl / 4;
  f.n_raw = n_raw;
  if (n_raw == 0) return CMGPU_OK;
  if (f.keep.ensure(((size_t)n_raw + 1) * 4) || f.pos.ensure(((size_t)n_raw + 1) * 4) || f.recidx.ensure((size_t)n_raw * 4) || f.bad.ensure(8) ||
      f.scan_tmp.ensure(cm_scan_tmp_words(n_raw) * 4)) { cm_set_error(c, "out of device memory (FASTQ records)"); return CMGPU_ENOMEM; }
  const uint32_t none = 0xffffffffu;
  CM_HIPCHECK(c, hipMemsetAsync(f.bad.p, 0xff, 8, s));
  const dim3 gr((n_raw + FQ_BLOCK - 1) / FQ_BLOCK);
  hipLaunchKernelGGL(k_fq_records, gr, b, 0, s, (const uint8_t *)f.text.p, (const uint32_t *)f.nl.p, n_raw,
                     free_layout ? 3 : stream == 2 || f.keep_reads ? 1 : 0,  // (FREE: a quality of another length is kseq's -2 for every stream)
                     (uint32_t *)f.keep.p, (uint32_t *)f.bad.p);
  cm_scan_u32((const uint32_t *)f.keep.p, (uint32_t *)f.pos.p, n_raw, (uint32_t *)f.scan_tmp.p, s);
  hipLaunchKernelGGL(k_fq_compact, gr, b, 0, s, (const uint32_t *)f.keep.p, (const uint32_t *)f.pos.p, n_raw, (uint32_t *)f.recidx.p);
  uint32_t bad = 0, bad_q = 0, n_rec = 0;
  CM_HIPCHECK(c, hipMemcpyAsync(&bad, f.bad.p, 4, hipMemcpyDeviceToHost, s));
  CM_HIPCHECK(c, hipMemcpyAsync(&bad_q, (uint32_t *)f.bad.p + 1, 4, hipMemcpyDeviceToHost, s));
  CM_HIPCHECK(c, hipMemcpyAsync(&n_rec, (uint32_t *)f.pos.p + n_raw, 4, hipMemcpyDeviceToHost, s));
  CM_HIPCHECK(c, cm_stream_sync(s));
  if (bad != none && free_layout) return fq_scan_general(c, stream, n_lines, final_chunk != 0, unterminated, n_records);
  if (bad != none && bad == bad_q && stream != 2) {  // (only seen with keep_reads on: the qualities of reads are not looked at otherwise)
    cm_set_error(c, "truncated quality: the quality line is not as long as the sequence at record " + std::to_string(bad) +
                        " of the chunk (whole reads are kept for SAM output, cmgpu_fastq_keep_reads)");
    f.n_raw = 0;
    return CMGPU_EFORMAT;
  }
  if (bad != none) {
    cm_set_error(c, "not a 4-line FASTQ record (missing '@' / '+' marker or quality length) at record " + std::to_string(bad) + " of the chunk");
    f.n_raw = 0;
    return CMGPU_EFORMAT;
  }
  if (free_layout && n_rec) {  // (four-line records have their quality)
    f.fx_seen |= CM_FX_SEEN_FASTQ;
    if (f.fx_seen == (CM_FX_SEEN_FASTQ | CM_FX_SEEN_FASTA)) {
      cm_set_error(c, "records with quality and records without in one stream: FASTA and FASTQ mixed, or a FASTQ file cut short inside a record (corrupted?)");
      f.n_raw = 0;
      return CMGPU_EFORMAT;
    }
  }
  f.n_rec = n_rec;
  *n_records = n_rec;
  return CMGPU_OK;
}

// ---------------------------------------------------------------------------------------
// BGZF input inflated on the device (the reference: one zlib gzread per file, sequence_batch.cc:22-62).
// The host walks the block headers (18 bytes each: the 'BC' field holds the block's size) and uploads the COMPRESSED bytes.
// k_bgzf_tokens: a lane per block decodes its DEFLATE codes (cm_inflate.h pass 1) -- literals straight to the block's place in the
// stream's text (the ISIZE trailers give the places), matches as tokens; k_bgzf_resolve: a wave per block with the block's text in
// LDS copies the matches, checks the CRC-32 and writes the text back.  The text then stays on the device: what cmgpu_fastq_take
// does not consume is kept in front of the next blocks (the host never sees inflated bytes and cannot resubmit them).
// ---------------------------------------------------------------------------------------
struct FqBgzfBlock { uint32_t coff, clen, ooff, isize, crc, toff; };
#define FQ_INF_LANES 64
#define FQ_INF_STEPS 2048u  // symbols per lane between two header phases of the wave
__global__ __launch_bounds__(FQ_INF_LANES) void k_bgzf_tokens(const uint8_t *__restrict__ comp, const FqBgzfBlock *__restrict__ tab, uint32_t n_blocks,
                                                                uint8_t *__restrict__ text, uint32_t *__restrict__ tok, uint32_t *__restrict__ ntok,
                                                                uint32_t *__restrict__ status) {
  __shared__ uint16_t sym[CM_INF_SYMS * FQ_INF_LANES];
  __shared__ uint8_t len8[CM_INF_LENS * FQ_INF_LANES];
  __shared__ int16_t delta[32 * FQ_INF_LANES];
  const uint32_t bi = blockIdx.x * FQ_INF_LANES + threadIdx.x;
  const bool active = bi < n_blocks;  // (a lane without a block still walks the wave's phases)
  FqBgzfBlock b = {0, 0, 0, 0, 0, 0};
  if (active) b = tab[bi];
  uint32_t n = 0;
  const int rc = cm_inflate_tokens(comp + b.coff, b.clen, text + b.ooff, b.isize, tok + b.toff, &n, active, sym + threadIdx.x, len8 + threadIdx.x,
                                   delta + threadIdx.x, FQ_INF_LANES, FQ_INF_STEPS);
  if (!active) return;
  ntok[bi] = rc == CM_INF_OK ? n : 0xffffffffu;
  if (rc != CM_INF_OK) atomicMin(status, (bi << 3) | (uint32_t)rc);  // the first damaged block and what is wrong with it
}
// the group type cm_inflate.h's second pass asks for: one wave
struct FqWave {
  static constexpr int G = 64;
  uint32_t t;
  __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  __device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
  __device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }  // lane: uniform
  __device__ __forceinline__ uint32_t rank(bool p, uint32_t *total) {
    const unsigned long long m = __ballot(p);
    *total = (uint32_t)__popcll(m);
    return (uint32_t)__popcll(m & ((1ull << t) - 1ull));
  }
  __device__ __forceinline__ uint32_t scan(uint32_t v, uint32_t *total) {
    uint32_t incl = v;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      const uint32_t x = __shfl_up(incl, dlt, 64);
      if (t >= (uint32_t)dlt) incl += x;
    }
    *total = __shfl(incl, 63, 64);
    return incl - v;
  }
};
__global__ __launch_bounds__(64) void k_bgzf_resolve(const FqBgzfBlock *__restrict__ tab, uint8_t *__restrict__ text, const uint32_t *__restrict__ tok,
                                                     const uint32_t *__restrict__ ntok, CmCrcX2n x2n, uint32_t *__restrict__ status) {
  __shared__ uint4 win16[65536 / 16 + 2];
  __shared__ uint32_t ends[128];
  __shared__ uint32_t red[64], crc_tab[256], x2[32];
  FqWave g;
  g.t = threadIdx.x;
  const uint32_t bi = blockIdx.x;
  const uint32_t n_tok = ntok[bi];
  if (n_tok == 0xffffffffu) return;  // (pass 1 gave the block up)
  const FqBgzfBlock b = tab[bi];
  for (uint32_t i = g.t; i < 256; i += 64) crc_tab[i] = cm_crc32_entry(i);
  if (g.t < 32) x2[g.t] = x2n.v[g.t];
  // the block's text (literals in place) into LDS, 16 bytes per lane and step, at its alignment in the text
  const uint32_t a = b.ooff & 15u;
  const uint4 *src = reinterpret_cast<const uint4 *>(text + (b.ooff - a));
  const uint32_t n16 = (a + b.isize + 15u) / 16u;
  for (uint32_t i0 = 0; i0 < n16; i0 += 8u * 64u) {  // (eight loads in flight per lane: a load a step would wait out HBM's latency 64 times)
    uint4 r[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) { const uint32_t i = i0 + u * 64u + g.t; r[u] = src[i < n16 ? i : n16 - 1u]; }
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) { const uint32_t i = i0 + u * 64u + g.t; win16[i < n16 ? i : 65536u / 16u + 1u] = r[u]; }  // (the last word: nobody's)
  }
  g.sync();
  uint8_t *win = reinterpret_cast<uint8_t *>(win16) + a;
  int rc = cm_bgzf_resolve(g, win, tok + b.toff, n_tok, b.isize, ends);
  if (rc == CM_INF_OK && cm_bgzf_crc(g, win, b.isize, crc_tab, x2, red) != b.crc) rc = CM_INF_ECRC;
  if (rc != CM_INF_OK) { if (g.t == 0) atomicMin(status, (bi << 3) | (uint32_t)rc); return; }
  // back to the text: whole 16-byte pieces inside the block, its first and last bytes one by one (the neighbours' are not ours)
  uint4 *dst = reinterpret_cast<uint4 *>(text + (b.ooff - a));
  const uint32_t first16 = a ? 1u : 0u, end16 = (a + b.isize) / 16u;
  for (uint32_t i0 = first16; i0 < end16; i0 += 4u * 64u) {
    uint4 r[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) { const uint32_t i = i0 + u * 64u + g.t; r[u] = win16[i < end16 ? i : first16]; }
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) { const uint32_t i = i0 + u * 64u + g.t; if (i < end16) dst[i] = r[u]; }
  }
  const uint32_t head = a ? (16u - a < b.isize ? 16u - a : b.isize) : 0u;
  if (g.t < head) text[b.ooff + g.t] = win[g.t];
  const uint32_t tail_at = end16 * 16u > a + head ? end16 * 16u - a : head;  // first byte after the whole pieces
  if (tail_at + g.t < b.isize) text[b.ooff + tail_at + g.t] = win[tail_at + g.t];
}
// the stream's text buffer with room for `need` bytes, the first `keep` bytes preserved
static int fq_text_room(cmgpu_ctx *c, CmFqStream &f, uint64_t need, uint64_t keep) {
  if (f.text.cap >= need) return CMGPU_OK;
  DevBuf bigger;
  if (bigger.ensure(need + need / 4)) { cm_set_error(c, "out of device memory (FASTQ text)"); return CMGPU_ENOMEM; }
  {
    hipError_t e = keep ? hipMemcpyAsync(bigger.p, f.text.p, keep, hipMemcpyDeviceToDevice, fq_hs(c, f)) : hipSuccess;
    if (e == hipSuccess) e = cm_stream_sync(fq_hs(c, f));
    if (e != hipSuccess) { bigger.release(); CM_HIPCHECK(c, e); }
  }
  f.text.release();
  f.text = bigger;
  bigger.p = nullptr; bigger.cap = 0;
  return CMGPU_OK;
}
// after a take in device mode: the unconsumed rest of the text moves to the front (through the second buffer: the ranges may overlap)
static int fq_retain_rest(cmgpu_ctx *c, CmFqStream &f, uint64_t consumed, bool end_of_file, uint64_t *consumed_out) {
  uint64_t rest = f.n_bytes > consumed ? f.n_bytes - consumed : 0;
  if (end_of_file && rest) {
    // every record of the file is taken: what follows the last one may only be blank (the host check of a plain-text file:
    // "Didn't reach the end of sequence file"); it is dropped so that the next file starts on an empty text
    // (the whole tail, 64 KiB at a time: a file may end in any amount of blank lines, as the host path's only_whitespace() accepts)
    std::vector<char> tail(rest < 65536 ? rest : 65536);
    bool blank = true;
    for (uint64_t o = 0; blank && o < rest; o += tail.size()) {
      const size_t m = rest - o < tail.size() ? (size_t)(rest - o) : tail.size();
      CM_HIPCHECK(c, hipMemcpyAsync(tail.data(), (const uint8_t *)f.text.p + consumed + o, m, hipMemcpyDeviceToHost, fq_hs(c, f)));
      CM_HIPCHECK(c, cm_stream_sync(fq_hs(c, f)));
      for (size_t i = 0; i < m; ++i) { const char ch = tail[i]; blank = blank && (ch == '\n' || ch == '\r' || ch == ' ' || ch == '\t'); }
    }
    if (!blank) { cm_set_error(c, "text after the last whole FASTQ record of the file"); return CMGPU_EFORMAT; }
    consumed += rest;  // (the blank tail counts as consumed: the caller's byte accounting ends at the file's end)
    if (consumed_out) *consumed_out = consumed;
    rest = 0;
  }
  if (rest) {
    // (sized like the first buffer: the two swap, and a buffer that is large enough is left alone)
    if (f.text2.cap < rest + 32 && f.text2.ensure(rest + 32 > f.text.cap ? rest + 32 : f.text.cap)) { cm_set_error(c, "out of device memory (FASTQ text)"); return CMGPU_ENOMEM; }
    CM_HIPCHECK(c, hipMemcpyAsync(f.text2.p, (const uint8_t *)f.text.p + consumed, rest, hipMemcpyDeviceToDevice, fq_hs(c, f)));
    CM_HIPCHECK(c, cm_stream_sync(fq_hs(c, f)));
    DevBuf t = f.text; f.text = f.text2; f.text2 = t;
  }
  f.dev_len = rest;
  f.n_bytes = rest; f.n_nl = 0; f.n_raw = 0; f.n_rec = 0;  // (the retained text is scanned again with the next blocks)
  return CMGPU_OK;
}
extern "C" int cmgpu_fastq_scan_bgzf(cmgpu_ctx *c, int stream, const void *blocks, uint64_t n_bytes, int final_chunk, uint32_t *n_records) {
  if (!c || stream < 0 || stream > 2 || (!blocks && n_bytes) || !n_records) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  CmFqStream &f = c->fq[stream];
  hipStream_t s = fq_hs(c, f);
  *n_records = 0;
  if (!f.dev_mode) { f.dev_mode = true; f.dev_len = 0; }
  // ---- the blocks' table (host): whole blocks only
  const uint8_t *p = static_cast<const uint8_t *>(blocks);
  std::vector<FqBgzfBlock> tab;
  uint64_t at = 0, out = f.dev_len, n_tok_cap = 0;
  while (at < n_bytes) {
    if (n_bytes - at < 28 || p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8 || !(p[at + 3] & 4) || p[at + 10] != 6 || p[at + 11] != 0 ||
        p[at + 12] != 'B' || p[at + 13] != 'C' || p[at + 14] != 2 || p[at + 15] != 0) {
      cm_set_error(c, "not a BGZF block at byte " + std::to_string((unsigned long long)at) + " of the chunk"); return CMGPU_EFORMAT;
    }
    const uint64_t bsize = ((uint64_t)p[at + 16] | ((uint64_t)p[at + 17] << 8)) + 1;
    if (bsize < 28 || bsize > n_bytes - at) { cm_set_error(c, "truncated BGZF block at byte " + std::to_string((unsigned long long)at) + " of the chunk"); return CMGPU_EFORMAT; }
    const uint8_t *t = p + at + bsize - 8;
    const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    if (isize > 65536u) { cm_set_error(c, "BGZF block larger than 64 KiB at byte " + std::to_string((unsigned long long)at) + " of the chunk"); return CMGPU_EFORMAT; }
    if (out + isize > 0xfffffff0ull) { cm_set_error(c, "FASTQ chunk must be smaller than 4 GiB"); return CMGPU_EINVAL; }
    if (isize) { tab.push_back({(uint32_t)(at + 18), (uint32_t)(bsize - 26), (uint32_t)out, isize, crc, (uint32_t)n_tok_cap}); n_tok_cap += cm_inf_tok_cap(isize); }
    out += isize;
    at += bsize;
  }
  if (n_bytes > 0xfffffff0ull) { cm_set_error(c, "BGZF chunk must be smaller than 4 GiB"); return CMGPU_EINVAL; }
  // ---- upload, inflate behind the text kept from the last take
  int rc = fq_text_room(c, f, out + 32, f.dev_len);
  if (rc) return rc;
  if (!tab.empty()) {
    if (f.comp.ensure(n_bytes + 16) || f.btab.ensure(tab.size() * sizeof(FqBgzfBlock)) || f.bad.ensure(4) || f.toks.ensure((size_t)n_tok_cap * 4) ||
        f.ntok.ensure(tab.size() * 4)) {
      cm_set_error(c, "out of device memory (BGZF blocks)"); return CMGPU_ENOMEM;
    }
    static const CmCrcX2n x2n = []() { CmCrcX2n x; cm_crc_x2n_table(x); return x; }();
    const uint32_t none = 0xffffffffu;
    CM_HIPCHECK(c, hipMemcpyAsync(f.comp.p, blocks, n_bytes, hipMemcpyHostToDevice, s));
    CM_HIPCHECK(c, hipMemcpyAsync(f.btab.p, tab.data(), tab.size() * sizeof(FqBgzfBlock), hipMemcpyHostToDevice, s));
    CM_HIPCHECK(c, hipMemcpyAsync(f.bad.p, &none, 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_bgzf_tokens, dim3((unsigned)((tab.size() + FQ_INF_LANES - 1) / FQ_INF_LANES)), dim3(FQ_INF_LANES), 0, s,
                       (const uint8_t *)f.comp.p, (const FqBgzfBlock *)f.btab.p, (uint32_t)tab.size(), (uint8_t *)f.text.p, (uint32_t *)f.toks.p,
                       (uint32_t *)f.ntok.p, (uint32_t *)f.bad.p);
    hipLaunchKernelGGL(k_bgzf_resolve, dim3((unsigned)tab.size()), dim3(64), 0, s, (const FqBgzfBlock *)f.btab.p, (uint8_t *)f.text.p,
                       (const uint32_t *)f.toks.p, (const uint32_t *)f.ntok.p, x2n, (uint32_t *)f.bad.p);
    uint32_t st = 0;
    CM_HIPCHECK(c, hipMemcpyAsync(&st, f.bad.p, 4, hipMemcpyDeviceToHost, s));
    CM_HIPCHECK(c, cm_stream_sync(s));
    if (st != none) {
      static const char *what[] = {"", "the stream runs past the block's end", "the inflated size differs from the block's ISIZE", "invalid code", "CRC mismatch"};
      cm_set_error(c, std::string("damaged BGZF block ") + std::to_string(st >> 3) + " of the chunk (" + what[(st & 7) < 5 ? (st & 7) : 3] + ")");
      return CMGPU_EFORMAT;
    }
  }
  f.dev_len = out;
  f.n_bytes = out; f.n_nl = 0; f.n_raw = 0; f.n_rec = 0; f.final_chunk = final_chunk != 0;
  f.general = false; f.fx_lines = 0; f.fx_stop = 0;
  if (out == 0) return CMGPU_OK;
  char last_char = 0;
  CM_HIPCHECK(c, hipMemcpyAsync(&last_char, (const uint8_t *)f.text.p + out - 1, 1, hipMemcpyDeviceToHost, s));
  CM_HIPCHECK(c, cm_stream_sync(s));
  return fq_scan_resident(c, stream, out, final_chunk, last_char, n_records);
}

// (everything here runs on the FASTQ stream's own HIP stream and writes the STAGING buffers st_*: a caller may take the next batch while
//  another of its threads is inside cmgpu_map_resident / cmgpu_store_append_resident with the committed one -- no null-stream call, which
//  would wait for the mapping stream, and no hipFree, which waits for the device)
extern "C" int cmgpu_fastq_take(cmgpu_ctx *c, int stream, uint32_t n, uint64_t *bytes_consumed) {
  if (!c || stream < 0 || stream > 2 || !bytes_consumed) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  CmFqStream &f = c->fq[stream];
  hipStream_t s = fq_hs(c, f);
  if (n > f.n_rec) { cm_set_error(c, "more records requested than the chunk holds"); return CMGPU_EINVAL; }
  DevBuf &bases = stream == 0 ? c->st_rb0 : stream == 1 ? c->st_rb1 : c->st_bcb;
  DevBuf &offs = stream == 0 ? c->st_ro0 : stream == 1 ? c->st_ro1 : c->st_bco;
  if (f.final_chunk && n == f.n_rec) f.fx_seen = 0;  // (the file ends with this take: the next one may hold the other kind of records)
  f.taken = n;
  f.taken_bases = 0;
  f.taken_max_len = 0;
  f.taken_name_bytes = 0;
  const bool names = f.keep_names || f.keep_reads, reads = f.keep_reads && stream < 2;
  // where the host resumes: the end of the last raw record used; trailing empty records and,
  // at the end of the file, blank lines go with it
  uint32_t last_raw = 0;
  bool have_last = false;
  if (f.general) {}
  else if (n == f.n_rec) { if (f.n_raw) { last_raw = f.n_raw - 1; have_last = true; } }
  else if (n > 0) {
    CM_HIPCHECK(c, hipMemcpyAsync(&last_raw, (uint32_t *)f.recidx.p + (n - 1), 4, hipMemcpyDeviceToHost, s));
    CM_HIPCHECK(c, cm_stream_sync(s));
    have_last = true;
  }
  uint64_t consumed = 0;
  if (f.general) {
    // the line where seek state stands behind the taken records: where the countable records end, or the line after the last one taken
    uint32_t line = f.fx_stop;
    if (n < f.n_rec && n > 0) {
      CM_HIPCHECK(c, hipMemcpyAsync(&last_raw, (uint32_t *)f.recidx.p + (n - 1), 4, hipMemcpyDeviceToHost, s));
      CM_HIPCHECK(c, cm_stream_sync(s));
      CM_HIPCHECK(c, hipMemcpyAsync(&line, (uint32_t *)f.fx_nxt.p + last_raw, 4, hipMemcpyDeviceToHost, s));
      CM_HIPCHECK(c, cm_stream_sync(s));
    } else if (n < f.n_rec) line = 0;
    if (line > 0) {
      uint32_t endnl = 0;
      CM_HIPCHECK(c, hipMemcpyAsync(&endnl, (uint32_t *)f.nl.p + (line - 1), 4, hipMemcpyDeviceToHost, s));
      CM_HIPCHECK(c, cm_stream_sync(s));
      consumed = (uint64_t)endnl + 1;
      if (consumed > f.n_bytes) consumed = f.n_bytes;
    }
  }
  if (have_last) {
    uint32_t endnl = 0;
    CM_HIPCHECK(c, hipMemcpyAsync(&endnl, (uint32_t *)f.nl.p + (4 * (size_t)last_raw + 3), 4, hipMemcpyDeviceToHost, s));
    CM_HIPCHECK(c, cm_stream_sync(s));
    consumed = (uint64_t)endnl + 1;
    if (consumed > f.n_bytes) consumed = f.n_bytes;
  }
  *bytes_consumed = consumed;
  if (offs.ensure(((size_t)n + 1) * 4)) { cm_set_error(c, "out of device memory (read offsets)"); return CMGPU_ENOMEM; }
  if (n == 0) {
    CM_HIPCHECK(c, hipMemsetAsync(offs.p, 0, 4, s));
    CM_HIPCHECK(c, cm_stream_sync(s));
    return f.dev_mode ? fq_retain_rest(c, f, consumed, f.final_chunk && n == f.n_rec, bytes_consumed) : CMGPU_OK;
  }
  if (f.len.ensure(((size_t)n + 1) * 4) || f.scan_tmp.ensure(cm_scan_tmp_words(n) * 4) || f.bad.ensure(4) ||
      (names && (f.nm_len.ensure(((size_t)n + 1) * 4) || f.nm_off.ensure(((size_t)n + 1) * 4)))) {
    cm_set_error(c, "out of device memory (FASTQ lengths)"); return CMGPU_ENOMEM;
  }
  const dim3 g((n + FQ_BLOCK - 1) / FQ_BLOCK), b(FQ_BLOCK);
  FqFormat fmt;
  fmt.n_ranges = f.n_ranges;
  for (int k = 0; k < 4; ++k) { fmt.start[k] = f.rng_start[k]; fmt.end[k] = f.rng_end[k]; }
  fmt.minus = f.minus ? 1 : 0;
  if (f.general) hipLaunchKernelGGL(k_fx_len, g, b, 0, s, (const uint32_t *)f.fx_sl.p, (const uint32_t *)f.recidx.p, n, fmt, (uint32_t *)f.len.p);
  else hipLaunchKernelGGL(k_fq_len, g, b, 0, s, (const uint8_t *)f.text.p, (const uint32_t *)f.nl.p, (const uint32_t *)f.recidx.p, n, fmt, (uint32_t *)f.len.p);
  cm_scan_u32((const uint32_t *)f.len.p, (uint32_t *)offs.p, n, (uint32_t *)f.scan_tmp.p, s);
  size_t tb = 0;
  (void)rocprim::reduce(nullptr, tb, (const uint32_t *)f.len.p, (uint32_t *)f.bad.p, 0u, (size_t)n, FqMaxOp(), s);
  if (f.red_tmp.ensure(tb + 256)) { cm_set_error(c, "out of device memory (reduce)"); return CMGPU_ENOMEM; }
  hipError_t e = rocprim::reduce(f.red_tmp.p, tb, (const uint32_t *)f.len.p, (uint32_t *)f.bad.p, 0u, (size_t)n, FqMaxOp(), s);
  uint32_t total = 0, mx = 0, name_total = 0;
  if (names) {  // (lengths and offsets of the names in the same wait as the bases')
    if (f.general) hipLaunchKernelGGL(k_fq_name_len<true>, g, b, 0, s, (const uint8_t *)f.text.p, f.n_bytes, (const uint32_t *)f.nl.p, (const uint32_t *)f.recidx.p, n,
                                      (uint32_t *)f.nm_len.p);
    else hipLaunchKernelGGL(k_fq_name_len<false>, g, b, 0, s, (const uint8_t *)f.text.p, f.n_bytes, (const uint32_t *)f.nl.p, (const uint32_t *)f.recidx.p, n,
                            (uint32_t *)f.nm_len.p);
    cm_scan_u32((const uint32_t *)f.nm_len.p, (uint32_t *)f.nm_off.p, n, (uint32_t *)f.scan_tmp.p, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&name_total, (uint32_t *)f.nm_off.p + n, 4, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&total, (uint32_t *)offs.p + n, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&mx, f.bad.p, 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = cm_stream_sync(s);
  if (e != hipSuccess) { cm_set_error(c, std::string("FASTQ take: ") + hipGetErrorString(e)); return CMGPU_EHIP; }
  if (bases.ensure((size_t)total + 16) || (stream == 2 && c->st_bcq.ensure((size_t)total + 16))) { cm_set_error(c, "out of device memory (reads)"); return CMGPU_ENOMEM; }
  if (names && f.st_nm.ensure((size_t)name_total + 16)) { cm_set_error(c, "out of device memory (read names)"); return CMGPU_ENOMEM; }
  if (reads && f.st_q.ensure((size_t)total + 16)) { cm_set_error(c, "out of device memory (read qualities)"); return CMGPU_ENOMEM; }
  uint8_t *quals = stream == 2 ? (uint8_t *)c->st_bcq.p : reads ? (uint8_t *)f.st_q.p : (uint8_t *)nullptr;
  if (f.general)
    hipLaunchKernelGGL(k_fx_gather, g, b, 0, s, (const uint8_t *)f.text.p, (const uint32_t *)f.nl.p, (const uint32_t *)f.fx_nxt.p, (const uint32_t *)f.fx_send.p,
                       (const uint32_t *)f.fx_sl.p, (const uint32_t *)f.recidx.p, (const uint32_t *)offs.p, n, fmt, (uint8_t *)bases.p, quals);
  else
    hipLaunchKernelGGL(k_fq_gather, g, b, 0, s, (const uint8_t *)f.text.p, (const uint32_t *)f.nl.p, (const uint32_t *)f.recidx.p,
                       (const uint32_t *)offs.p, n, fmt, (uint8_t *)bases.p, quals);
  if (names && f.general)
    hipLaunchKernelGGL(k_fq_name_gather<true>, g, b, 0, s, (const uint8_t *)f.text.p, (const uint32_t *)f.nl.p, (const uint32_t *)f.recidx.p,
                       (const uint32_t *)f.nm_off.p, n, (uint8_t *)f.st_nm.p);
  else if (names)
    hipLaunchKernelGGL(k_fq_name_gather<false>, g, b, 0, s, (const uint8_t *)f.text.p, (const uint32_t *)f.nl.p, (const uint32_t *)f.recidx.p,
                       (const uint32_t *)f.nm_off.p, n, (uint8_t *)f.st_nm.p);
  CM_HIPCHECK(c, cm_stream_sync(s));
  f.taken_bases = total;
  f.taken_max_len = mx;
  f.taken_name_bytes = name_total;
  if (f.dev_mode) return fq_retain_rest(c, f, consumed, f.final_chunk && n == f.n_rec, bytes_consumed);
  return CMGPU_OK;
}

// ---- the run-wide name store: blob + 64-bit offsets indexed by read_id - nm_base, doubling like the record store (cm_post.hip) ----
static int fq_names_reserve(cmgpu_ctx *c, CmFqStream &f, uint64_t need_n, uint64_t need_bytes) {
  hipStream_t s = fq_hs(c, f);
  if (need_n > c->nm_cap_n || !c->nm_offs.p) {
    uint64_t cap = c->nm_cap_n ? c->nm_cap_n * 2 : 1u << 20;
    if (cap < need_n) cap = need_n;
    DevBuf nb;
    if (nb.ensure((cap + 1) * 8)) { cm_set_error(c, "out of device memory (read-name store: offsets of " + std::to_string((unsigned long long)cap) + " names)"); return CMGPU_ENOMEM; }
    hipError_t e = c->nm_offs.p ? hipMemcpyAsync(nb.p, c->nm_offs.p, (c->nm_n + 1) * 8, hipMemcpyDeviceToDevice, s) : hipMemsetAsync(nb.p, 0, 8, s);
    if (e == hipSuccess) e = cm_stream_sync(s);
    if (e != hipSuccess) { nb.release(); CM_HIPCHECK(c, e); }
    c->nm_offs.release();
    c->nm_offs = nb;
    c->nm_cap_n = cap;
  }
  if (need_bytes + 16 > c->nm_blob.cap) {
    uint64_t cap = c->nm_blob.cap ? c->nm_blob.cap * 2 : 32u << 20;
    if (cap < need_bytes + 16) cap = need_bytes + 16;
    DevBuf nb;
    // (ensure() asks for a quarter more than it is told and falls back to the bare size)
    if (nb.ensure(cap)) { cm_set_error(c, "out of device memory (read-name store: " + std::to_string((unsigned long long)cap) + " bytes of names)"); return CMGPU_ENOMEM; }
    hipError_t e = c->nm_bytes ? hipMemcpyAsync(nb.p, c->nm_blob.p, c->nm_bytes, hipMemcpyDeviceToDevice, s) : hipSuccess;
    if (e == hipSuccess) e = cm_stream_sync(s);
    if (e != hipSuccess) { nb.release(); CM_HIPCHECK(c, e); }
    c->nm_blob.release();
    c->nm_blob = nb;
  }
  return CMGPU_OK;
}
// the n names last taken from f (staging) behind the store's; they must continue it: first_read_id == nm_base + nm_n
static int fq_names_append(cmgpu_ctx *c, CmFqStream &f, uint32_t n, uint32_t first_read_id) {
  if (c->nm_n == 0) c->nm_base = first_read_id;
  else if ((uint64_t)first_read_id != (uint64_t)c->nm_base + c->nm_n) {
    cm_set_error(c, "read names are kept for consecutive read ids: the store ends at read " + std::to_string((unsigned long long)c->nm_base + c->nm_n) +
                        ", the batch starts at " + std::to_string(first_read_id) + " (cmgpu_names_clear starts a new run)");
    return CMGPU_EINVAL;
  }
  if (n == 0) return CMGPU_OK;
  const int rc = fq_names_reserve(c, f, c->nm_n + n, c->nm_bytes + f.taken_name_bytes);
  if (rc) return rc;
  hipStream_t s = fq_hs(c, f);
  hipLaunchKernelGGL(k_fq_name_append, dim3(n / FQ_BLOCK + 1), dim3(FQ_BLOCK), 0, s, (const uint32_t *)f.nm_off.p, n, c->nm_bytes,
                     (uint64_t *)c->nm_offs.p + c->nm_n);
  if (f.taken_name_bytes)
    CM_HIPCHECK(c, hipMemcpyAsync((uint8_t *)c->nm_blob.p + c->nm_bytes, f.st_nm.p, f.taken_name_bytes, hipMemcpyDeviceToDevice, s));
  CM_HIPCHECK(c, cm_stream_sync(s));
  c->nm_n += n;
  c->nm_bytes += f.taken_name_bytes;
  return CMGPU_OK;
}

// ---- the run-wide read store (cmgpu_fastq_keep_reads): per mate names / bases / qualities with 64-bit offsets, indexed by read_id - rd_base ----
int cm_grow_buf(cmgpu_ctx *c, DevBuf &b, uint64_t used, uint64_t need, uint64_t first, hipStream_t s, const char *what) {
  if (need <= b.cap && b.p) return CMGPU_OK;
  uint64_t cap = b.cap ? (uint64_t)b.cap * 2 : first;
  if (cap < need) cap = need;
  DevBuf nb;
  if (nb.ensure(cap)) { cm_set_error(c, std::string("out of device memory (") + what + ": " + std::to_string((unsigned long long)cap) + " bytes)"); return CMGPU_ENOMEM; }
  hipError_t e = used && b.p ? hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, s) : hipSuccess;
  if (e == hipSuccess) e = cm_stream_sync(s);
  if (e != hipSuccess) { nb.release(); CM_HIPCHECK(c, e); }
  b.release();
  b = nb;
  return CMGPU_OK;
}
// room for the batch last taken (n records per mate) behind the store's reads; changes no count
static int fq_reads_reserve(cmgpu_ctx *c, int mates, uint32_t n) {
  for (int m = 0; m < mates; ++m) {
    CmFqStream &f = c->fq[m];
    CmReadMate &r = c->rd[m];
    hipStream_t s = fq_hs(c, f);
    const uint64_t have = c->rd_n ? (c->rd_n + 1) * 8 : 0, want = (c->rd_n + n + 1) * 8;
    int rc = cm_grow_buf(c, r.name_offs, have, want, 8u << 20, s, "read store: name offsets");
    if (!rc) rc = cm_grow_buf(c, r.offs, have, want, 8u << 20, s, "read store: base offsets");
    if (!rc) rc = cm_grow_buf(c, r.names, r.name_bytes, r.name_bytes + f.taken_name_bytes + 16, 32u << 20, s, "read store: names");
    if (!rc) rc = cm_grow_buf(c, r.bases, r.base_bytes, r.base_bytes + f.taken_bases + 16, 128u << 20, s, "read store: bases");
    if (!rc) rc = cm_grow_buf(c, r.quals, r.base_bytes, r.base_bytes + f.taken_bases + 16, 128u << 20, s, "read store: qualities");
    if (rc) return rc;
  }
  return CMGPU_OK;
}
// the batch last taken (staging buffers: the commit has not swapped them yet) behind the store's reads; first_read_id == rd_base + rd_n
static int fq_reads_append(cmgpu_ctx *c, int mates, uint32_t n, uint32_t first_read_id) {
  if (c->rd_n && ((uint64_t)first_read_id != (uint64_t)c->rd_base + c->rd_n || c->rd_paired != (mates == 2))) {
    cm_set_error(c, "reads are kept for consecutive read ids of one kind of batch: the store ends at read " + std::to_string((unsigned long long)c->rd_base + c->rd_n) +
                        ", the batch starts at " + std::to_string(first_read_id) + " (cmgpu_reads_clear starts a new run)");
    return CMGPU_EINVAL;
  }
  if (n == 0) return CMGPU_OK;
  const int rc = fq_reads_reserve(c, mates, n);
  if (rc) return rc;
  for (int m = 0; m < mates; ++m) {
    CmFqStream &f = c->fq[m];
    CmReadMate &r = c->rd[m];
    hipStream_t s = fq_hs(c, f);
    const DevBuf &sb = m == 0 ? c->st_rb0 : c->st_rb1, &so = m == 0 ? c->st_ro0 : c->st_ro1;
    const dim3 g(n / FQ_BLOCK + 1), b(FQ_BLOCK);
    hipLaunchKernelGGL(k_fq_name_append, g, b, 0, s, (const uint32_t *)f.nm_off.p, n, r.name_bytes, (uint64_t *)r.name_offs.p + c->rd_n);
    hipLaunchKernelGGL(k_fq_name_append, g, b, 0, s, (const uint32_t *)so.p, n, r.base_bytes, (uint64_t *)r.offs.p + c->rd_n);
    if (f.taken_name_bytes) CM_HIPCHECK(c, hipMemcpyAsync((uint8_t *)r.names.p + r.name_bytes, f.st_nm.p, f.taken_name_bytes, hipMemcpyDeviceToDevice, s));
    if (f.taken_bases) {
      CM_HIPCHECK(c, hipMemcpyAsync((uint8_t *)r.bases.p + r.base_bytes, sb.p, f.taken_bases, hipMemcpyDeviceToDevice, s));
      CM_HIPCHECK(c, hipMemcpyAsync((uint8_t *)r.quals.p + r.base_bytes, f.st_q.p, f.taken_bases, hipMemcpyDeviceToDevice, s));
    }
  }
  for (int m = 0; m < mates; ++m) CM_HIPCHECK(c, cm_stream_sync(fq_hs(c, c->fq[m])));
  if (c->rd_n == 0) { c->rd_base = first_read_id; c->rd_paired = mates == 2; }
  for (int m = 0; m < mates; ++m) { c->rd[m].name_bytes += c->fq[m].taken_name_bytes; c->rd[m].base_bytes += c->fq[m].taken_bases; }
  c->rd_n += n;
  return CMGPU_OK;
}

// declares the records taken from the streams the resident batch (what cmgpu_upload_batch does
// for host SoA buffers); cmgpu_map_resident maps it
extern "C" int cmgpu_fastq_commit(cmgpu_ctx *c, uint32_t n, uint32_t first_read_id, int paired, int barcoded) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  if (c->fq[0].taken != n || (paired && c->fq[1].taken != n) || (barcoded && c->fq[2].taken != n)) {
    cm_set_error(c, "streams hold different numbers of taken records"); return CMGPU_EINVAL;
  }
  if (n > 0x3fffffffu) { cm_set_error(c, "batch too large"); return CMGPU_EINVAL; }
  if (barcoded && c->wl_size != 0 && c->wl_num_sample == 0) { cm_set_error(c, "barcode abundance not computed"); return CMGPU_EINVAL; }
  // the batch's names join the run-wide store first: a commit that cannot keep them (a gap in the read ids, no memory) changes nothing
  for (int m = 0; m < 2; ++m)
    if (c->fq[m].keep_names) {
      if (m == 1 && !paired) { cm_set_error(c, "the names of read 2 are kept, but the batch is single-end"); return CMGPU_EINVAL; }
      const int nrc = fq_names_append(c, c->fq[m], n, first_read_id);
      if (nrc) return nrc;
    }
  if (c->fq[0].keep_reads) {  // (likewise the whole reads; names and reads exclude each other, so at most one store is written)
    const int rrc = fq_reads_append(c, paired ? 2 : 1, n, first_read_id);
    if (rrc) return rrc;
  }
  // the taken batch becomes the resident one: the staging buffers and the resident batch's swap (the old batch's buffers take the next
  // take).  The caller has no cmgpu_map_* call of this context running here.
  std::swap(c->rb0, c->st_rb0); std::swap(c->ro0, c->st_ro0);
  if (paired) { std::swap(c->rb1, c->st_rb1); std::swap(c->ro1, c->st_ro1); }
  if (barcoded) { std::swap(c->bcb, c->st_bcb); std::swap(c->bcq, c->st_bcq); std::swap(c->bco, c->st_bco); }
  c->n_pairs = n;
  c->first_read_id = first_read_id;
  c->single = !paired;
  c->has_barcodes = barcoded != 0;
  c->bases0 = c->fq[0].taken_bases;
  c->bases1 = paired ? c->fq[1].taken_bases : 0;
  uint32_t mx = c->fq[0].taken_max_len;
  if (paired && c->fq[1].taken_max_len > mx) mx = c->fq[1].taken_max_len;
  c->max_read_len = mx ? mx : 1;
  if (!paired) {
    if (c->ro1.ensure(((size_t)n + 1) * 4) || c->rb1.ensure(16)) { cm_set_error(c, "out of device memory (reads)"); return CMGPU_ENOMEM; }
    CM_HIPCHECK(c, hipMemset(c->ro1.p, 0, ((size_t)n + 1) * 4));
  }
  return CMGPU_OK;
}

// Replaces kseq's name.s for the device ingest (kseq.h:188, read into SequenceBatch by LoadOneSequenceAndSaveAt, sequence_batch.cc:36):
// the stream's takes also gather the records' names.  One stream per context: the store is indexed by read id.
extern "C" int cmgpu_fastq_keep_names(cmgpu_ctx *c, int stream, int on) {
  if (!c || stream < 0 || stream > 1) return CMGPU_EINVAL;
  if (on && c->fq[0].keep_reads) { cm_set_error(c, "whole reads are kept already (cmgpu_fastq_keep_reads): their names are among them"); return CMGPU_EINVAL; }
  if (on && c->fq[1 - stream].keep_names) { cm_set_error(c, "the names of one stream are kept per context (those of the other mate are already on)"); return CMGPU_EINVAL; }
  c->fq[stream].keep_names = on != 0;
  c->fq[stream].taken_name_bytes = 0;
  return CMGPU_OK;
}
extern "C" int cmgpu_names_clear(cmgpu_ctx *c) {
  if (!c) return CMGPU_EINVAL;
  c->nm_n = 0;
  c->nm_bytes = 0;
  c->nm_base = 0;
  return CMGPU_OK;
}
extern "C" int cmgpu_names_info(const cmgpu_ctx *c, uint64_t *n_names, uint64_t *n_bytes, uint32_t *read_id_base) {
  if (!c) return CMGPU_EINVAL;
  if (n_names) *n_names = c->nm_n;
  if (n_bytes) *n_bytes = c->nm_bytes;
  if (read_id_base) *read_id_base = c->nm_base;
  return CMGPU_OK;
}
extern "C" int cmgpu_download_names(cmgpu_ctx *c, char *blob, uint64_t blob_capacity, uint64_t *offsets) {
  if (!c || !offsets || (!blob && c->nm_bytes)) return CMGPU_EINVAL;
  if (blob_capacity < c->nm_bytes) { cm_set_error(c, "name buffer too small"); return CMGPU_ECAPACITY; }
  CM_HIPCHECK(c, cm_enter(c));
  offsets[0] = 0;
  if (c->nm_n) CM_HIPCHECK(c, hipMemcpy(offsets, c->nm_offs.p, (c->nm_n + 1) * 8, hipMemcpyDeviceToHost));
  if (c->nm_bytes) CM_HIPCHECK(c, hipMemcpy(blob, c->nm_blob.p, c->nm_bytes, hipMemcpyDeviceToHost));
  return CMGPU_OK;
}

// Replaces, for the device ingest, what SequenceBatch::LoadOneSequenceAndSaveAt keeps of a record for SAM output (sequence_batch.cc:22-62: name,
// sequence, quality): the takes of read 1 and read 2 gather all three, the commit appends them to the read store.
extern "C" int cmgpu_fastq_keep_reads(cmgpu_ctx *c, int on) {
  if (!c) return CMGPU_EINVAL;
  if (on && (c->fq[0].keep_names || c->fq[1].keep_names)) { cm_set_error(c, "read names are kept already (cmgpu_fastq_keep_names): keep either names or whole reads"); return CMGPU_EINVAL; }
  for (int m = 0; m < 2; ++m) { c->fq[m].keep_reads = on != 0; c->fq[m].taken_name_bytes = 0; }
  return CMGPU_OK;
}
extern "C" int cmgpu_reads_clear(cmgpu_ctx *c) {
  if (!c) return CMGPU_EINVAL;
  c->rd_n = 0;
  c->rd_base = 0;
  c->rd_paired = false;
  for (CmReadMate &r : c->rd) { r.name_bytes = 0; r.base_bytes = 0; }
  return CMGPU_OK;
}
extern "C" int cmgpu_reads_info(const cmgpu_ctx *c, int mate, uint64_t *n_reads, uint64_t *name_bytes, uint64_t *base_bytes, uint32_t *read_id_base) {
  if (!c || mate < 0 || mate > 1) return CMGPU_EINVAL;
  const bool has = mate == 0 || c->rd_paired;
  if (n_reads) *n_reads = has ? c->rd_n : 0;
  if (name_bytes) *name_bytes = c->rd[mate].name_bytes;
  if (base_bytes) *base_bytes = c->rd[mate].base_bytes;
  if (read_id_base) *read_id_base = c->rd_base;
  return CMGPU_OK;
}
extern "C" int cmgpu_download_reads(cmgpu_ctx *c, int mate, char *names, uint64_t names_capacity, uint64_t *name_offsets, char *bases, char *quals,
                                    uint64_t bases_capacity, uint64_t *offsets) {
  if (!c || mate < 0 || mate > 1 || !name_offsets || !offsets) return CMGPU_EINVAL;
  const CmReadMate &r = c->rd[mate];
  const uint64_t n = mate == 0 || c->rd_paired ? c->rd_n : 0;
  if ((!names && r.name_bytes) || ((!bases || !quals) && r.base_bytes)) return CMGPU_EINVAL;
  if (names_capacity < r.name_bytes || bases_capacity < r.base_bytes) { cm_set_error(c, "read buffer too small"); return CMGPU_ECAPACITY; }
  CM_HIPCHECK(c, cm_enter(c));
  name_offsets[0] = 0;
  offsets[0] = 0;
  if (n) {
    CM_HIPCHECK(c, hipMemcpy(name_offsets, r.name_offs.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    CM_HIPCHECK(c, hipMemcpy(offsets, r.offs.p, (n + 1) * 8, hipMemcpyDeviceToHost));
  }
  if (r.name_bytes) CM_HIPCHECK(c, hipMemcpy(names, r.names.p, r.name_bytes, hipMemcpyDeviceToHost));
  if (r.base_bytes) {
    CM_HIPCHECK(c, hipMemcpy(bases, r.bases.p, r.base_bytes, hipMemcpyDeviceToHost));
    CM_HIPCHECK(c, hipMemcpy(quals, r.quals.p, r.base_bytes, hipMemcpyDeviceToHost));
  }
  return CMGPU_OK;
}

// --read-format for one stream: n_ranges (0..4) [start, end] pairs (end = -1: up to the last base), strand '+' or '-'
extern "C" int cmgpu_fastq_set_format(cmgpu_ctx *c, int stream, int n_ranges, const int32_t *starts, const int32_t *ends, char strand) {
  if (!c || stream < 0 || stream > 2 || n_ranges < 0 || n_ranges > 4 || (n_ranges && (!starts || !ends)) || (strand != '+' && strand != '-')) return CMGPU_EINVAL;
  CmFqStream &f = c->fq[stream];
  f.n_ranges = n_ranges;
  for (int k = 0; k < n_ranges; ++k) { f.rng_start[k] = starts[k]; f.rng_end[k] = ends[k]; }
  f.minus = strand == '-';
  // the full range on the + strand is the identity (IsFullRangeAndPositiveStrand)
  if (n_ranges >= 1 && !f.minus && starts[0] == 0 && ends[0] == -1) f.n_ranges = 0;
  return CMGPU_OK;
}

// Record layout of one stream (cm_fastx.h): CMGPU_FASTX_FREE reads what kseq_read reads (kseq.h:177-218); the default stays four-line FASTQ
extern "C" int cmgpu_fastq_set_layout(cmgpu_ctx *c, int stream, int layout) {
  if (!c || stream < 0 || stream > 2) return CMGPU_EINVAL;
  if (layout != CMGPU_FASTX_STRICT4 && layout != CMGPU_FASTX_FREE) { cm_set_error(c, "unknown FASTQ record layout " + std::to_string(layout)); return CMGPU_EINVAL; }
  CmFqStream &f = c->fq[stream];
  if (layout != f.layout && f.dev_mode && f.dev_len) {
    cm_set_error(c, "the record layout cannot change while text of the stream is kept on the device (cmgpu_fastq_scan_bgzf)");
    return CMGPU_EINVAL;
  }
  f.layout = layout;
  f.fx_seen = 0;
  return CMGPU_OK;
}
extern "C" int cmgpu_fastq_scan_info(const cmgpu_ctx *c, int stream, int *general_path, uint32_t *n_lines) {
  if (!c || stream < 0 || stream > 2) return CMGPU_EINVAL;
  const CmFqStream &f = c->fq[stream];
  if (general_path) *general_path = f.general ? 1 : 0;
  if (n_lines) *n_lines = f.general ? f.fx_lines : f.n_nl;
  return CMGPU_OK;
}

// the device code of this translation unit is loaded by the HIP runtime at the first launch of one of its kernels (milliseconds to tens of
// milliseconds for the larger ones): context creation launches this empty kernel so that a job's first batch does not pay for it (cm_api.hip: cm_load_device_code)
__global__ void k_touch_ingest() {}
void cm_touch_ingest(hipStream_t s) { hipLaunchKernelGGL(k_touch_ingest, dim3(1), dim3(1), 0, s); }
