// cm_tabix.h -- the tabix index (.tbi; SAM/tabix spec, preset `bed`) of a sorted BED / TagAlign text that cm_bgzf_out.hip has compressed:
// what a line, a raw chunk, a tile of the text and the finished index need, written so that the device (cm_tabix.hip) and a host
// without one (tests/hostemu/hostemu_tabix.cpp) run the same functions.  Block k of the compressed store holds the text bytes
// [k * 0xff00, (k + 1) * 0xff00); coff[k] is its offset in the store and `base` the file offset of the store's first block, so the
// virtual offset of text byte u is ((base + coff[u / 0xff00]) << 16) | (u % 0xff00), and that of the text's end the first byte
// behind the last block.
//  1. line starts: the newlines of every tile of CM_TBX_TILE bytes counted (cm_tbx_tile_count), the counts scanned, the starts
//     scattered (cm_tbx_tile_starts).  A group of lanes works a tile: piece q of 16 bytes is lane q % G's in round q / G.
//  2. per line: columns 1-3 parsed and validated, column 1 compared with the line above (cm_tbx_line_parse); after a scan of the
//     head flags, reference, bin, sortedness and the head flag of (reference, bin) (cm_tbx_line_flags); after a scan of those, the raw
//     chunks and the linear index's minima (cm_tbx_line_emit).  The first offending line: one 64-bit minimum of line << 3 | cause.
//  3. per raw chunk, sorted by (reference, bin) with a stable sort: it joins the chunk before it when it begins in the block in
//     which that one ends (cm_tbx_chunk_flag), then the merged chunks (cm_tbx_chunk_emit).
//  4. the payload, on the host, from arrays as long as the index (cm_tbx_serialize).
// The CSI index (.csi; SAM spec 5.3, CSIv1) is the same index with the number of levels as a parameter: min_shift stays 14 (the 16 kb
// windows above), depth is 1 .. 6 and the limit of an end 2^(14 + 3 * depth).  Positions are 32-bit here, so depth 6 accepts ends up
// to 0xffffffff, not 2^32.  CmTbxArrays::csi_depth (and CmBaiArrays') says which: 0 is the .tbi / .bai scheme -- depth 5, limit
// 2^29, keys reference << 16 | bin -- and 1 .. 6 the CSI's with keys reference << 20 | bin (depth 6 has bins up to 299 592).  A
// CSI has no linear index: every bin carries `loffset`, the back-filled window value at the bin's first position
// (cm_csi_bin_loffset, per merged chunk that is the first of its bin); the windows themselves stay where they were made.
//  4c. the CSI payload, on the host, for both flavours (cm_csi_serialize): BAM (no aux) and tabix (aux: the tabix header's fields).
// The functions that write a shared word take the way to do it as a template argument `A` (min64): atomics on the device,
// plain code on the host.
#ifndef CM_TABIX_H_
#define CM_TABIX_H_
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "cm_types.h"

#define CM_TBX_SLICE 0xff00u
#define CM_TBX_TILE 4096u    // bytes of text per tile
#define CM_TBX_PIECE 16u     // bytes a lane looks at in one go
#define CM_TBX_MAX_END (1u << 29)
#define CM_TBX_PSEUDO_BIN 37450u
#define CM_TBX_KEY_SHIFT 16u  // the chunk key of the .tbi / .bai: reference << 16 | bin
#define CM_CSI_KEY_SHIFT 20u  // ... of the .csi
#define CM_CSI_MIN_SHIFT 14u
#define CM_CSI_MAX_DEPTH 6u
#define CM_TBX_MAX_LINES 0xfffffffeull
// why a text cannot be indexed (the low three bits of the error word)
#define CM_TBX_E_MALFORMED 1u  // fewer than three columns, an empty name, a column 2 or 3 that is not decimal
#define CM_TBX_E_RECUR 2u      // a name heads a second run of lines (found on the host, among the names)
#define CM_TBX_E_UNSORTED 3u   // a start smaller than the line's above, same name
#define CM_TBX_E_RANGE 4u      // an end beyond 2^29 (beyond the depth's limit for a CSI)
#define CM_TBX_NO_ERROR (~0ull)

struct CmTbxText {
  const uint8_t *p;
  uint64_t n;             // bytes; the last one is a newline
  uint64_t n_blocks;
  const uint64_t *coff;   // n_blocks + 1
  uint64_t base;
};
struct CmTbxRef {  // one run of lines with the same column 1
  uint64_t vbeg, vend;   // virtual offsets of its first line's start and its last line's end
  uint64_t name_at;      // text offset of its name
  uint32_t first_line, name_len, n_intv, pad;
};
struct CmTbxChunk { uint64_t key, beg, end; };  // key: reference << 16 | bin (CSI: reference << 20 | bin)
struct CmTbxArrays {
  CmTbxText t;
  uint64_t n_lines;
  const uint64_t *lstart;   // n_lines + 1: where every line starts, and the text's end
  uint32_t *beg, *end;      // per line; end > beg
  uint32_t *tid;            // per line: 1 where column 1 differs from the line's above; after the scan 1 + reference
  uint32_t *cidx;           // per line: 1 where (reference, bin) differs from the line's above; after the scan 1 + raw chunk
  unsigned long long *err;  // the smallest line << 3 | cause
  CmTbxRef *ref;
  const uint64_t *lin_off;  // per reference: where its windows begin in lin
  unsigned long long *lin;  // per window of 16 kb: the smallest virtual offset of a line that overlaps it
  uint64_t *ckey, *cbeg, *cend;  // per raw chunk, in text order
  uint32_t *cval;                // per raw chunk: its own number (the sort carries it)
  uint32_t csi_depth;            // 0: the .tbi's scheme; 1 .. 6: a CSI of that depth
};

CM_HD uint64_t cm_tbx_voff(const CmTbxText &t, uint64_t u) {
  if (u >= t.n) return (t.base + t.coff[t.n_blocks]) << 16;
  const uint64_t k = u / CM_TBX_SLICE;
  return ((t.base + t.coff[k]) << 16) | (u - k * CM_TBX_SLICE);
}
CM_HD uint32_t cm_tbx_reg2bin(uint32_t beg, uint32_t end) {
  --end;
  if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
  if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
  if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
  if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
  if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
  return 0;
}
// ---- the CSI's scheme: min_shift 14, `depth` levels below bin 0 (1 .. 6)
// the specification's reg2bin for [beg, end), end > beg; depth 5 gives cm_tbx_reg2bin
CM_HD uint32_t cm_csi_reg2bin(uint32_t beg, uint32_t end, uint32_t depth) {
  uint32_t l = depth, s = CM_CSI_MIN_SHIFT, t = ((1u << (3u * depth)) - 1u) / 7u;
  for (--end; l > 0; --l, s += 3u, t -= 1u << (3u * l))
    if (beg >> s == end >> s) return t + (beg >> s);
  return 0;
}
CM_HD uint32_t cm_csi_pseudo_bin(uint32_t depth) { return ((1u << (3u * depth + 3u)) - 1u) / 7u + 1u; }
// the largest end a record may have: 2^(14 + 3 * depth), and 0xffffffff at depth 6 (32-bit positions)
CM_HD uint64_t cm_csi_max_end(uint32_t depth) {
  const uint64_t lim = 1ull << (CM_CSI_MIN_SHIFT + 3u * depth);
  return lim > 0xffffffffull ? 0xffffffffull : lim;
}
// the 16 kb window in which bin `bin` begins: the levels walked from the top, at most `depth` steps
CM_HD uint64_t cm_csi_bin_window(uint32_t bin, uint32_t depth) {
  uint32_t l = 0, first = 0;  // first: the first bin of level l
  while (l < depth && bin >= first + (1u << (3u * l))) { first += 1u << (3u * l); ++l; }
  return (uint64_t)(bin - first) << (3u * (depth - l));
}
// what a zero-initialised struct means: the .tbi / .bai scheme
CM_HD uint32_t cm_tbx_depth_of(uint32_t csi_depth) { return csi_depth ? csi_depth : 5u; }
CM_HD uint32_t cm_tbx_key_shift_of(uint32_t csi_depth) { return csi_depth ? CM_CSI_KEY_SHIFT : CM_TBX_KEY_SHIFT; }
// a bin's loffset (htslib's rule): the back-filled window value at the bin's first position.  The bin exists because a record lies
// in it, so the window is one of its reference's, and after the back-fill it is not all ones
CM_HD uint64_t cm_csi_bin_loffset(uint64_t key, uint32_t depth, const unsigned long long *lin, const uint64_t *lin_off) {
  const uint64_t ref = key >> CM_CSI_KEY_SHIFT;
  return lin[lin_off[ref] + cm_csi_bin_window((uint32_t)(key & ((1u << CM_CSI_KEY_SHIFT) - 1u)), depth)];
}

// ---- 1. line starts
// bit i: text[off + i] is a newline (i < 16, off + i < n)
CM_HD uint32_t cm_tbx_nl_mask(const uint8_t *text, uint64_t off, uint64_t n) {
  uint32_t m = 0;
  if (off + CM_TBX_PIECE <= n && (reinterpret_cast<uintptr_t>(text + off) & 7u) == 0) {
    const uint64_t *w = reinterpret_cast<const uint64_t *>(text + off);
    for (int h = 0; h < 2; ++h) {
      const uint64_t y = w[h] ^ 0x0a0a0a0a0a0a0a0aull, k = 0x7f7f7f7f7f7f7f7full;
      const uint64_t z = ~(((y & k) + k) | y | k);  // 0x80 in every byte of y that is zero, exactly
      m |= (uint32_t)(((z >> 7) * 0x0102040810204080ull) >> 56) << (8 * h);
    }
    return m;
  }
  for (uint32_t i = 0; i < CM_TBX_PIECE && off + i < n; ++i) m |= (text[off + i] == '\n' ? 1u : 0u) << i;
  return m;
}
// the newlines of tile `tile`, the same in every lane
template <class GT>
CM_HD uint32_t cm_tbx_tile_count(GT &g, const uint8_t *text, uint64_t n, uint64_t tile) {
  uint32_t mine = 0;
  for (uint32_t q = g.t; q < CM_TBX_TILE / CM_TBX_PIECE; q += (uint32_t)GT::G)
    mine += (uint32_t)__builtin_popcount(cm_tbx_nl_mask(text, tile * CM_TBX_TILE + (uint64_t)q * CM_TBX_PIECE, n));
  return g.sum(mine);
}
// lstart[j + 1] = one past newline j, for the newlines of the tile; `first` newlines lie before it
template <class GT>
CM_HD void cm_tbx_tile_starts(GT &g, const uint8_t *text, uint64_t n, uint64_t tile, uint64_t first, uint64_t *lstart) {
  uint64_t at = first;
  for (uint32_t r = 0; r < CM_TBX_TILE / CM_TBX_PIECE; r += (uint32_t)GT::G) {  // (every lane takes part in every round's scan)
    const uint32_t q = r + g.t;
    const uint64_t off = tile * CM_TBX_TILE + (uint64_t)q * CM_TBX_PIECE;
    uint32_t m = q < CM_TBX_TILE / CM_TBX_PIECE ? cm_tbx_nl_mask(text, off, n) : 0u;
    uint32_t tot;
    uint64_t j = at + g.scan((uint32_t)__builtin_popcount(m), &tot);
    for (; m; m &= m - 1u) lstart[++j] = off + (uint32_t)__builtin_ctz(m) + 1u;
    at += tot;
  }
}

// ---- 2. per line
// decimal digits from p on, at most up to le; a value beyond 2^33 stays there
CM_HD uint64_t cm_tbx_number(const uint8_t *text, uint64_t &p, uint64_t le, uint32_t *n_digits) {
  uint64_t v = 0;
  uint32_t nd = 0;
  for (; p < le && text[p] >= '0' && text[p] <= '9'; ++p, ++nd) {
    v = v * 10u + (uint32_t)(text[p] - '0');
    if (v > (1ull << 33)) v = 1ull << 33;
  }
  *n_digits = nd;
  return v;
}
// the line [s, e) (e: one past its newline): 0 and [beg, end) -- end made beg + 1 where it is not larger -- and the length of
// column 1, or the cause it cannot be indexed for, with [0, 1).  max_end: the largest end the scheme takes
CM_HD uint32_t cm_tbx_columns(const uint8_t *text, uint64_t s, uint64_t e, uint32_t *beg, uint32_t *end, uint32_t *name_len,
                              uint64_t max_end = CM_TBX_MAX_END) {
  const uint64_t le = e - 1;
  uint64_t p = s;
  while (p < le && text[p] != '\t') ++p;
  *name_len = (uint32_t)(p - s);
  *beg = 0;
  *end = 1;
  if (p == s || p >= le) return CM_TBX_E_MALFORMED;
  ++p;
  uint32_t nd;
  const uint64_t b = cm_tbx_number(text, p, le, &nd);
  if (!nd || p >= le || text[p] != '\t') return CM_TBX_E_MALFORMED;
  ++p;
  uint64_t x = cm_tbx_number(text, p, le, &nd);
  if (!nd || (p < le && text[p] != '\t')) return CM_TBX_E_MALFORMED;
  if (x <= b) x = b + 1;
  if (x > max_end) return CM_TBX_E_RANGE;
  *beg = (uint32_t)b;
  *end = (uint32_t)x;
  return 0;
}
// the line at s has the name_len bytes of column 1 of the line at s_prev (which ends at s) as its own column 1
CM_HD bool cm_tbx_same_name(const uint8_t *text, uint64_t s_prev, uint64_t s, uint32_t name_len) {
  if (s_prev + name_len >= s - 1 || text[s_prev + name_len] != '\t') return false;
  for (uint32_t i = 0; i < name_len; ++i)
    if (text[s_prev + i] != text[s + i]) return false;
  return true;
}
// line i: beg, end, the head flag of its name
template <class A>
CM_HD void cm_tbx_line_parse(const CmTbxArrays &d, uint64_t i) {
  const uint64_t s = d.lstart[i], e = d.lstart[i + 1];
  uint32_t beg, end, name_len;
  const uint32_t cause = cm_tbx_columns(d.t.p, s, e, &beg, &end, &name_len, cm_csi_max_end(cm_tbx_depth_of(d.csi_depth)));
  if (cause) A::min64(d.err, (unsigned long long)i << 3 | cause);
  d.beg[i] = beg;
  d.end[i] = end;
  d.tid[i] = i == 0 || !cm_tbx_same_name(d.t.p, d.lstart[i - 1], s, name_len) ? 1u : 0u;
}
// line i, tid scanned: sortedness, the head flag of (reference, bin), what its reference has to know.  Returns the windows the line
// asks of its reference's linear index; *ref_of its reference (the caller raises CmTbxRef::n_intv: a wave does it for all its lanes);
// *err_mine: the line's error word, where it has one (the caller lowers *d.err)
CM_HD uint32_t cm_tbx_line_flags_core(const CmTbxArrays &d, uint64_t i, uint32_t *ref_of, unsigned long long *err_mine) {
  const uint32_t t = d.tid[i] - 1u, beg = d.beg[i], end = d.end[i];
  const bool head = i == 0 || d.tid[i - 1] != d.tid[i];
  const bool tail = i + 1 == d.n_lines || d.tid[i + 1] != d.tid[i];
  bool chead = head;
  if (!head) {
    if (beg < d.beg[i - 1]) *err_mine = (unsigned long long)i << 3 | CM_TBX_E_UNSORTED;
    const uint32_t depth = cm_tbx_depth_of(d.csi_depth);
    chead = cm_csi_reg2bin(beg, end, depth) != cm_csi_reg2bin(d.beg[i - 1], d.end[i - 1], depth);
  }
  d.cidx[i] = chead ? 1u : 0u;
  CmTbxRef &r = d.ref[t];
  if (head) {
    const uint64_t s = d.lstart[i];
    uint64_t p = s;
    while (p < d.lstart[i + 1] - 1 && d.t.p[p] != '\t') ++p;
    r.vbeg = cm_tbx_voff(d.t, s);
    r.name_at = s;
    r.first_line = (uint32_t)i;
    r.name_len = (uint32_t)(p - s);
  }
  if (tail) r.vend = cm_tbx_voff(d.t, d.lstart[i + 1]);
  *ref_of = t;
  return ((end - 1u) >> 14) + 1u;
}
// line i, cidx scanned: the raw chunk it begins and the one it ends, and its start's virtual offset as a candidate for the windows
// it overlaps.  (The first window is left out where the line above lies in it too: that line's offset is the smaller one.)
template <class A>
CM_HD void cm_tbx_line_emit(const CmTbxArrays &d, uint64_t i) {
  const uint32_t t = d.tid[i] - 1u, ci = d.cidx[i] - 1u, beg = d.beg[i], end = d.end[i];
  const bool head = i == 0 || d.tid[i - 1] != d.tid[i];
  const uint64_t vs = cm_tbx_voff(d.t, d.lstart[i]);
  if (i == 0 || d.cidx[i - 1] != d.cidx[i]) {
    d.ckey[ci] = (uint64_t)t << cm_tbx_key_shift_of(d.csi_depth) | cm_csi_reg2bin(beg, end, cm_tbx_depth_of(d.csi_depth));
    d.cbeg[ci] = vs;
    d.cval[ci] = ci;
  }
  if (i + 1 == d.n_lines || d.cidx[i + 1] != d.cidx[i]) d.cend[ci] = cm_tbx_voff(d.t, d.lstart[i + 1]);
  uint32_t w = beg >> 14;
  const uint32_t w1 = (end - 1u) >> 14;
  if (!head && d.beg[i - 1] >> 14 == w) ++w;
  unsigned long long *lin = d.lin + d.lin_off[t];
  for (; w <= w1; ++w) A::min64(lin + w, vs);
}

// ---- 3. per raw chunk, sorted: key[j] and the chunk's number perm[j]
CM_HD uint32_t cm_tbx_chunk_flag(const uint64_t *key, const uint32_t *perm, const uint64_t *cbeg, const uint64_t *cend, uint64_t j) {
  return j == 0 || key[j] != key[j - 1] || cbeg[perm[j]] >> 16 > cend[perm[j - 1]] >> 16 ? 1u : 0u;
}
// midx: the flags scanned (1 + merged chunk)
CM_HD void cm_tbx_chunk_emit(const uint64_t *key, const uint32_t *perm, const uint64_t *cbeg, const uint64_t *cend, const uint32_t *midx, uint64_t n,
                             uint64_t j, CmTbxChunk *out) {
  const uint32_t m = midx[j] - 1u;
  if (j == 0 || midx[j - 1] != midx[j]) { out[m].key = key[j]; out[m].beg = cbeg[perm[j]]; }
  if (j + 1 == n || midx[j + 1] != midx[j]) out[m].end = cend[perm[j]];
}

// ---- 4. the payload (host)
static inline void cm_tbx_put(std::vector<uint8_t> &o, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; ++i) o.push_back((uint8_t)(v >> (8 * i)));
}
// names: the references' names back to back, name_off their n_ref + 1 offsets; ch: the merged chunks in (reference, bin, file) order;
// lin: all references' windows, back-filled
static inline void cm_tbx_serialize(const CmTbxRef *ref, uint32_t n_ref, uint64_t n_lines, const uint8_t *names, const uint64_t *name_off,
                                    const CmTbxChunk *ch, uint64_t n_ch, const uint64_t *lin, const uint64_t *lin_off, std::vector<uint8_t> &o) {
  o.clear();
  o.reserve(64 + (n_ref ? name_off[n_ref] + n_ref : 0) + (size_t)n_ref * 48 + n_ch * 24 + (n_ref ? lin_off[n_ref] * 8 : 0));
  const uint8_t magic[4] = {'T', 'B', 'I', 1};
  o.insert(o.end(), magic, magic + 4);
  const uint32_t head[7] = {n_ref, 0x10000u, 1u, 2u, 3u, 35u, 0u};
  for (uint32_t v : head) cm_tbx_put(o, v, 4);
  cm_tbx_put(o, n_ref ? name_off[n_ref] + n_ref : 0, 4);
  for (uint32_t r = 0; r < n_ref; ++r) {
    o.insert(o.end(), names + name_off[r], names + name_off[r + 1]);
    o.push_back(0);
  }
  uint64_t at = 0;
  for (uint32_t r = 0; r < n_ref; ++r) {
    uint64_t to = at;
    uint32_t n_bin = 1;  // the pseudo-bin
    for (; to < n_ch && ch[to].key >> 16 == r; ++to)
      if (to == at || ch[to].key != ch[to - 1].key) ++n_bin;
    cm_tbx_put(o, n_bin, 4);
    while (at < to) {
      uint64_t e = at + 1;
      while (e < to && ch[e].key == ch[at].key) ++e;
      cm_tbx_put(o, ch[at].key & 0xffffu, 4);
      cm_tbx_put(o, e - at, 4);
      for (; at < e; ++at) { cm_tbx_put(o, ch[at].beg, 8); cm_tbx_put(o, ch[at].end, 8); }
    }
    cm_tbx_put(o, CM_TBX_PSEUDO_BIN, 4);
    cm_tbx_put(o, 2, 4);
    cm_tbx_put(o, ref[r].vbeg, 8);
    cm_tbx_put(o, ref[r].vend, 8);
    cm_tbx_put(o, (r + 1 < n_ref ? ref[r + 1].first_line : n_lines) - ref[r].first_line, 8);
    cm_tbx_put(o, 0, 8);
    cm_tbx_put(o, ref[r].n_intv, 4);
    for (uint64_t w = lin_off[r]; w < lin_off[r + 1]; ++w) cm_tbx_put(o, lin[w], 8);
  }
  cm_tbx_put(o, 0, 8);
}
// ---- 4c. the CSI payload (host), both flavours.  ref: one entry per reference (has == 0: no record, no bin); ch: the merged chunks
// in (reference, bin, file) order with keys reference << 20 | bin; loff[j]: the loffset of chunk j's bin where j is the bin's first
// chunk; aux: l_aux bytes (BAM flavour: none)
struct CmCsiRef {
  uint64_t vbeg, vend, n_mapped, n_unmapped;
  uint32_t has, pad;
};
static inline void cm_csi_serialize(uint32_t depth, const uint8_t *aux, uint32_t l_aux, const CmCsiRef *ref, uint32_t n_ref, const CmTbxChunk *ch, uint64_t n_ch,
                                    const uint64_t *loff, std::vector<uint8_t> &o) {
  o.clear();
  o.reserve(32 + l_aux + (size_t)n_ref * 56 + n_ch * 32);
  const uint8_t magic[4] = {'C', 'S', 'I', 1};
  o.insert(o.end(), magic, magic + 4);
  cm_tbx_put(o, CM_CSI_MIN_SHIFT, 4);
  cm_tbx_put(o, depth, 4);
  cm_tbx_put(o, l_aux, 4);
  if (l_aux) o.insert(o.end(), aux, aux + l_aux);
  cm_tbx_put(o, n_ref, 4);
  const uint64_t bin_mask = (1ull << CM_CSI_KEY_SHIFT) - 1u;
  uint64_t at = 0;
  for (uint32_t r = 0; r < n_ref; ++r) {
    if (!ref[r].has) {  // no record: no bin, not the pseudo-bin either
      cm_tbx_put(o, 0, 4);
      continue;
    }
    uint64_t to = at;
    uint32_t n_bin = 1;  // the pseudo-bin
    for (; to < n_ch && ch[to].key >> CM_CSI_KEY_SHIFT == r; ++to)
      if (to == at || ch[to].key != ch[to - 1].key) ++n_bin;
    cm_tbx_put(o, n_bin, 4);
    while (at < to) {
      uint64_t e = at + 1;
      while (e < to && ch[e].key == ch[at].key) ++e;
      cm_tbx_put(o, ch[at].key & bin_mask, 4);
      cm_tbx_put(o, loff[at], 8);
      cm_tbx_put(o, e - at, 4);
      for (; at < e; ++at) { cm_tbx_put(o, ch[at].beg, 8); cm_tbx_put(o, ch[at].end, 8); }
    }
    cm_tbx_put(o, cm_csi_pseudo_bin(depth), 4);
    cm_tbx_put(o, 0, 8);
    cm_tbx_put(o, 2, 4);
    cm_tbx_put(o, ref[r].vbeg, 8);
    cm_tbx_put(o, ref[r].vend, 8);
    cm_tbx_put(o, ref[r].n_mapped, 8);
    cm_tbx_put(o, ref[r].n_unmapped, 8);
  }
  cm_tbx_put(o, 0, 8);  // n_no_coor: no record without a position is written
}
// the tabix flavour's aux: the tabix header behind its magic and n_ref, with the values cm_tbx_serialize writes
static inline void cm_csi_tabix_aux(uint32_t n_ref, const uint8_t *names, const uint64_t *name_off, std::vector<uint8_t> &aux) {
  aux.clear();
  const uint32_t head[6] = {0x10000u, 1u, 2u, 3u, 35u, 0u};
  for (uint32_t v : head) cm_tbx_put(aux, v, 4);
  cm_tbx_put(aux, n_ref ? name_off[n_ref] + n_ref : 0, 4);
  for (uint32_t r = 0; r < n_ref; ++r) {
    aux.insert(aux.end(), names + name_off[r], names + name_off[r + 1]);
    aux.push_back(0);
  }
}
// the words for the limit of a scheme's ends: "2^29" for the .tbi / .bai and a CSI of depth 5
static inline std::string cm_csi_limit_words(uint32_t csi_depth) {
  const uint32_t depth = cm_tbx_depth_of(csi_depth);
  return depth == 6 ? std::string("4294967295 (32-bit positions)") : "2^" + std::to_string(CM_CSI_MIN_SHIFT + 3u * depth);
}
// the message for an error word
static inline const char *cm_tbx_cause(uint32_t cause) {
  return cause == CM_TBX_E_MALFORMED ? "is malformed: three tab-separated columns are needed, the first not empty, the second and third decimal"
       : cause == CM_TBX_E_RECUR    ? "begins a second run of lines for a name that had one already: the text is not sorted by name"
       : cause == CM_TBX_E_UNSORTED ? "starts before the line above it: the text is not sorted by start (paired TagAlign, pairs and SAM text is not)"
                                    : "ends beyond 2^29, the limit of the tabix format (tabix -C or --output-csi builds a .csi index for such a file)";
}
// ... for a CSI of the given depth
static inline std::string cm_csi_tbx_cause(uint32_t cause, uint32_t depth) {
  if (cause != CM_TBX_E_RANGE) return cm_tbx_cause(cause);
  return "ends beyond " + cm_csi_limit_words(depth) + ", the limit of a CSI index of depth " + std::to_string(depth);
}
#endif
