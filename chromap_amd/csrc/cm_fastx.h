// cm_fastx.h -- the record structure of FASTA / FASTQ text in any layout, as kseq_read reads it (kseq.h:177-218), over the LINES of a
// chunk.  Shared by the device ingest (cm_ingest.hip, layout CMGPU_FASTX_FREE) and the host build of the tests
// (tests/hostemu/hostemu_fastx.cpp): plain functions of a line index, no HIP call in here.
//
// kseq is a byte automaton; for text whose records start at line starts it is this automaton over a line's first byte:
//   seek      lines are skipped up to one that starts with '@' or '>' (kseq.h:183): the header; name = the bytes behind the marker up to
//             the first isspace() byte (kseq.h:188)
//   sequence  a '+' line ends the sequence and starts the quality; an '@' / '>' line ends the record without quality and is the next
//             header (kseq.h:194-199); an empty line is skipped; any other line is appended, its trailing '\r' dropped (kseq.h:141)
//   quality   the rest of the '+' line is ignored (kseq.h:211); lines are appended -- at least one -- until the quality is as long as the
//             sequence (kseq.h:213): such a line may start with '@', '+' or '>'.  Equal lengths end the record, anything else is kseq's
//             -2, "truncated quality" (kseq.h:212,216)
// Where the line automaton would differ from the byte automaton the text is REFUSED, never read differently:
//   * a skipped line in seek state that is not blank (kseq finds an '@' in the middle of such a line)
//   * a line that is exactly "\r" while the sequence or the quality is still empty (kseq.h:141 drops a trailing '\r' only from a string
//     longer than one byte, so that '\r' would become a base or a quality value; once something has been appended it is dropped, and
//     the line counts as empty here as there), or as the unterminated last line of a sequence
//   * (a choice, not a difference) records WITH quality and records WITHOUT in one file: kseq reads such a mix, and so does half a record
//     behind a FASTQ file's last whole one ("@name", a few bases, end of file: a FASTA record to kseq).  A stream that has shown both
//     kinds is refused; a file of either kind alone, whatever its markers, is read
//
// The record boundaries are a chain: whether an '@' line is a header depends on everything in front of it.  It is resolved without a
// serial walk over the lines:
//   1. cm_fx_line_info   per line: class of its first byte, length without '\r'
//   2. cm_fx_walk        per line, AS IF seek state reached it: a header candidate walks its own record (the lines of one record), a
//                        blank line steps to the next line, anything else is junk.  Result: nxt -- the line where seek state resumes
//                        -- and the record's description
//   3. the lines seek state really reaches are the chain 0 -> nxt[0] -> nxt[nxt[0]] ...  Per tile of CM_FX_TILE lines
//      cm_fx_tile_jump (pointer doubling, log2(tile) rounds) gives every line its first chain element behind the tile;
//      cm_fx_tile_entries follows those exits from tile to tile (one step per tile the chain touches); cm_fx_tile_members then walks each
//      tile from its entry
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CM_FX_HD __host__ __device__ __forceinline__
#else
#define CM_FX_HD static inline
#endif

#ifndef CM_FX_TILE                // (the host build of the tests also uses a tile of a few lines)
#define CM_FX_TILE 2048u          // lines per tile of the chain resolution (8 KiB of LDS)
#define CM_FX_TILE_ROUNDS 11      // log2(CM_FX_TILE): pointer doubling is done after that many rounds
#endif
#define CM_FX_LEN_MASK 0x0fffffffu  // line info / record word: low 28 bits a length, high 4 bits a class / status
#define CM_FX_NONE 0xffffffffu

// class of a line (by its first byte)
enum { CM_FX_EMPTY = 0, CM_FX_CR = 1 /* exactly "\r" */, CM_FX_BLANK = 2 /* isspace() bytes only */, CM_FX_HDR = 3 /* '>' */,
       CM_FX_PLUS = 4, CM_FX_OTHER = 5, CM_FX_HDR_AT = 6 /* '@' */ };
CM_FX_HD bool cm_fx_is_hdr(uint32_t cls) { return cls == CM_FX_HDR || cls == CM_FX_HDR_AT; }
// status of the record (or step) that starts at a line, were seek state to reach it
enum { CM_FX_FASTQ = 0,       // complete, with quality: sequence lines (h, seq_end), '+' line seq_end, quality lines (seq_end, nxt)
       CM_FX_FASTA = 1,       // complete, no quality: sequence lines (h, seq_end), nxt == seq_end is the next header or the end of the text
       CM_FX_SKIP = 2,        // a blank line: nxt = h + 1
       CM_FX_INCOMPLETE = 3,  // the chunk ends inside the record (never in a final chunk): the countable records end here
       CM_FX_TRUNC = 4,       // kseq's -2
       CM_FX_JUNK = 5,        // a line that is neither blank nor a header where a header is looked for (or a line / sequence of 2^28 bytes and more)
       CM_FX_KEPT_CR = 6 };   // a '\r' that kseq would keep as a base or a quality value
// kinds of records a stream has shown (bits): one stream holds records with quality or records without, not both -- see below
enum { CM_FX_SEEN_FASTQ = 1, CM_FX_SEEN_FASTA = 2 };

CM_FX_HD bool cm_fx_isspace(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

// line `line` of the text: class << 28 | length without the terminator and without one trailing '\r'
CM_FX_HD uint32_t cm_fx_line_info(const uint8_t *text, const uint32_t *nl, uint32_t line) {
  const uint32_t st = line == 0 ? 0u : nl[line - 1] + 1u, en = nl[line];
  if (en <= st) return (uint32_t)CM_FX_EMPTY << 28;
  const uint8_t c = text[st];
  uint32_t len = en - st;
  if (text[en - 1] == '\r') --len;
  if (len == 0) return (uint32_t)CM_FX_CR << 28;
  if (len > CM_FX_LEN_MASK) len = CM_FX_LEN_MASK;
  uint32_t cls = CM_FX_OTHER;
  if (c == '@') cls = CM_FX_HDR_AT;
  else if (c == '>') cls = CM_FX_HDR;
  else if (c == '+') cls = CM_FX_PLUS;
  else if (cm_fx_isspace(c)) {  // (only such lines are read to their end)
    uint32_t i = st + 1;
    while (i < en && cm_fx_isspace(text[i])) ++i;
    if (i == en) cls = CM_FX_BLANK;
  }
  return (cls << 28) | len;
}

// what starts at line h if seek state reaches it.  li: cm_fx_line_info of the chunk's n_lines lines; final_chunk: the text ends with the
// chunk; unterminated: its last line has no '\n'.  Out: *nxt (> h), *seq_end, *sl = status << 28 | sequence length.
CM_FX_HD void cm_fx_walk(const uint32_t *li, uint32_t n_lines, uint32_t h, bool final_chunk, bool unterminated, uint32_t *nxt, uint32_t *seq_end,
                         uint32_t *sl) {
  const uint32_t cls = li[h] >> 28;
  *seq_end = h + 1;
  *nxt = n_lines;  // (a status that ends the chain)
  if (!cm_fx_is_hdr(cls)) {
    if (cls <= CM_FX_BLANK) { *nxt = h + 1; *sl = (uint32_t)CM_FX_SKIP << 28; }
    else *sl = (uint32_t)CM_FX_JUNK << 28;
    return;
  }
  if ((li[h] & CM_FX_LEN_MASK) == CM_FX_LEN_MASK) { *sl = (uint32_t)CM_FX_JUNK << 28; return; }
  uint32_t i = h + 1, acc = 0;
  for (; i < n_lines; ++i) {
    const uint32_t c = li[i] >> 28, l = li[i] & CM_FX_LEN_MASK;
    if (cm_fx_is_hdr(c) || c == CM_FX_PLUS) break;
    // (a sequence line's first byte is read on its own, kseq.h:194-197: a "\r" that ends the text without '\n' stays as well)
    if (c == CM_FX_CR && (acc == 0 || (final_chunk && unterminated && i == n_lines - 1))) { *sl = (uint32_t)CM_FX_KEPT_CR << 28; return; }
    if (l == CM_FX_LEN_MASK || acc + l >= CM_FX_LEN_MASK) { *sl = (uint32_t)CM_FX_JUNK << 28; return; }
    acc += l;
  }
  *seq_end = i;
  if (i == n_lines) {  // the end of the text ends the record; the end of a chunk proves nothing
    *sl = ((uint32_t)(final_chunk ? CM_FX_FASTA : CM_FX_INCOMPLETE) << 28) | acc;
    return;
  }
  if (cm_fx_is_hdr(li[i] >> 28)) { *nxt = i; *sl = ((uint32_t)CM_FX_FASTA << 28) | acc; return; }
  // the '+' line.  Without its '\n' there is "no quality string" (kseq.h:212), whatever the sequence
  if (final_chunk && unterminated && i == n_lines - 1) { *sl = ((uint32_t)CM_FX_TRUNC << 28) | acc; return; }
  uint32_t j = i + 1, q = 0;
  do {
    if (j >= n_lines) {
      if (final_chunk) break;
      *sl = ((uint32_t)CM_FX_INCOMPLETE << 28) | acc;
      return;
    }
    const uint32_t c = li[j] >> 28, l = li[j] & CM_FX_LEN_MASK;
    if (c == CM_FX_CR && q == 0) { *sl = (uint32_t)CM_FX_KEPT_CR << 28; return; }
    q = l > CM_FX_LEN_MASK - q ? CM_FX_LEN_MASK : q + l;
    ++j;
  } while (q < acc);
  *nxt = q == acc ? j : n_lines;
  *sl = ((uint32_t)(q == acc ? CM_FX_FASTQ : CM_FX_TRUNC) << 28) | acc;
}

// One round of pointer doubling for line i of the tile [t0, t1): e[] (one word per line of the tile, first nxt[t0 + k]) moves to the first
// chain element at or behind t1.  Another lane may have moved e[e[k] - t0] already in the same round: every value it can hold is a later
// element of the same chain, so the fixed point -- all that is used -- is the same.  CM_FX_TILE_ROUNDS rounds reach it.
CM_FX_HD void cm_fx_tile_jump(uint32_t *e, uint32_t t0, uint32_t t1, uint32_t k) {
  const uint32_t v = e[k];
  if (v < t1) e[k] = e[v - t0];
}
// the chain from line 0 on, tile by tile: entry[t] = the chain's first element inside tile t (CM_FX_NONE: it passes over the tile).
// exit_[i]: the fixed point of cm_fx_tile_jump for line i.  One step per tile.
CM_FX_HD void cm_fx_tile_entries(const uint32_t *exit_, uint32_t n_lines, uint32_t *entry) {
  uint32_t cur = 0;
  while (cur < n_lines) {
    entry[cur / CM_FX_TILE] = cur;
    cur = exit_[cur];
  }
}

// the sequence (or quality) of a record: the lines [lb, le) without terminators and '\r', concatenated; the bytes of the --read-format
// ranges go to dst[o ..], reversed (and, for bases, complemented) for the '-' strand.  raw: the concatenation's length, l: the kept length.
// The ranges are those of k_fq_gather (SequenceEffectiveRange::Replace, sequence_effective_range.h:84-122).
CM_FX_HD void cm_fx_copy(const uint8_t *text, const uint32_t *nl, uint32_t lb, uint32_t le, uint32_t raw, int n_ranges, const int *r_start,
                         const int *r_end, int minus, bool complement, uint32_t o, uint32_t l, uint8_t *dst) {
  uint32_t w = 0;
  const int nr = n_ranges ? n_ranges : 1;
  for (int k = 0; k < nr; ++k) {
    int st = n_ranges ? r_start[k] : 0, en = n_ranges ? (r_end[k] == -1 ? (int)raw - 1 : r_end[k]) : (int)raw - 1;
    if (en >= (int)raw) en = (int)raw - 1;
    if (st < 0) st = 0;
    if (en < st) continue;
    uint32_t p = 0;  // place of the line's first byte in the concatenation
    for (uint32_t line = lb; line < le && p <= (uint32_t)en; ++line) {
      const uint32_t s = line == 0 ? 0u : nl[line - 1] + 1u;
      uint32_t e = nl[line];
      if (e > s && text[e - 1] == '\r') --e;
      const uint32_t len = e - s;
      if (len == 0) continue;
      const uint32_t lo = (uint32_t)st > p ? (uint32_t)st : p, hi = (uint32_t)en < p + len - 1 ? (uint32_t)en : p + len - 1;
      for (uint32_t x = lo; x <= hi && lo <= hi; ++x) {
        uint8_t c = text[s + (x - p)];
        if (complement) {  // Uint8ToChar(3 ^ CharToUint8(c))
          const uint8_t u = c & 0xDF;
          c = u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N';
        }
        const uint32_t idx = w + (x - (uint32_t)st);
        dst[minus ? o + (l - 1 - idx) : o + idx] = c;
      }
      p += len;
    }
    w += (uint32_t)(en - st + 1);
  }
}
// the members of the chain inside one tile, from the tile's entry `first` (cm_fx_tile_entries) up to the tile's end t1
template <class F>
CM_FX_HD void cm_fx_tile_members(const uint32_t *nxt, uint32_t first, uint32_t t1, F f) {
  for (uint32_t i = first; i < t1; i = nxt[i]) f(i);
}
