// cm_bam.h -- a BAM alignment record (SAM spec 4.2) from a record of the SAM record store and its read: what cm_sam_post.hip's
// k_bam_format writes for a selected record in place of k_sp_format's line, written so that the device and a host without one
// (tests/hostemu/hostemu_bam.cpp) run the same functions.
//
//   block_size 4 | refID 4 | pos 4 | l_read_name 1 | mapq 1 | bin 2 | n_cigar_op 2 | flag 2 | l_seq 4 | next_refID 4 | next_pos 4 | tlen 4
//   read_name NUL | CIGAR words (len << 4 | op, as the store holds them) | SEQ, 4 bits a base, high nibble first | QUAL, the character - 33
//   'N' 'M' C/S/I value | 'M' 'D' 'Z' MD NUL | 'C' 'B' 'Z' barcode NUL (a store with barcodes)
//
// A record starts wherever the one before ended, so every part begins at any byte offset.  A group of lanes writes a record: lane 0
// the fixed bytes, the NULs and the tags' heads, the whole group name, CIGAR, SEQ, QUAL, MD and the plain barcode -- single bytes up
// to the destination's next 4-byte boundary, then whole words, a word per lane and step (8 bases, or 4 qualities with their 33s
// taken off in one go), then the last bytes (cm_bam_spread, the scheme of cm_sam_post.hip's sp_copy).  The lanes share nothing and
// wait for nobody: what lands in memory does not depend on their order.  `GT` is the group: GT::G lanes, g.t this one.
// `R` is the record: rid, pos, mpos, nm, mrid, tlen, flag, n_cigar, md_len, mapq, strand, trim_len (cm_sam_post.hip: SpRec).
#ifndef CM_BAM_H_
#define CM_BAM_H_
#include <stdint.h>

#include "cm_types.h"

#define CM_BAM_NAME_MAX 254u  // l_read_name is one byte and counts the NUL

// the SAM specification's reg2bin for [beg, end), end > beg
CM_HD uint32_t cm_bam_reg2bin(uint32_t beg, uint32_t end) {
  --end;
  if (beg >> 14 == end >> 14) return ((1u << 15) - 1u) / 7u + (beg >> 14);
  if (beg >> 17 == end >> 17) return ((1u << 12) - 1u) / 7u + (beg >> 17);
  if (beg >> 20 == end >> 20) return ((1u << 9) - 1u) / 7u + (beg >> 20);
  if (beg >> 23 == end >> 23) return ((1u << 6) - 1u) / 7u + (beg >> 23);
  if (beg >> 26 == end >> 26) return ((1u << 3) - 1u) / 7u + (beg >> 26);
  return 0;
}
// reference bases the CIGAR covers: M, D, N, =, X
CM_HD uint32_t cm_bam_ref_len(const uint32_t *cg, uint32_t n_cigar) {
  uint32_t rl = 0;
  for (uint32_t t = 0; t < n_cigar; ++t) {
    const uint32_t op = cg[t] & 0xfu;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cg[t] >> 4;
  }
  return rl;
}
// l_seq: the SEQ length of the SAM line (cm_sam_post.hip: sp_seq_len) -- the CIGAR's query length (M, I, S, =, X), at most trim_len
CM_HD uint32_t cm_bam_seq_len(const uint32_t *cg, uint32_t n_cigar, uint32_t trim_len) {
  uint32_t ql = 0;
  for (uint32_t t = 0; t < n_cigar; ++t) {
    const uint32_t op = cg[t] & 0xfu;
    if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ql += cg[t] >> 4;
  }
  return ql < trim_len ? ql : trim_len;
}
// bytes of NM's value: samtools' choice of the smallest unsigned type
CM_HD uint32_t cm_bam_nm_bytes(uint32_t nm) { return nm < 256u ? 1u : nm < 65536u ? 2u : 4u; }

// bytes of the record, block_size included.  has_cb: the store holds barcodes; cb_len: bytes of the CB:Z value
template <class R>
CM_HD uint64_t cm_bam_record_size(const R &r, const uint32_t *cg, uint32_t name_len, bool has_cb, uint32_t cb_len) {
  const uint32_t sl = cm_bam_seq_len(cg, r.n_cigar, r.trim_len);
  return 4ull + 32u + (name_len + 1u) + 4u * r.n_cigar + (sl + 1u) / 2u + sl + (3u + cm_bam_nm_bytes(r.nm)) + (3u + r.md_len + 1u) +
         (has_cb ? 3u + cb_len + 1u : 0u);
}

// a base's place in "=ACMGRSVTWYHKDBN", upper or lower case; anything else is N's 15.  The 26 letters' values are the nibbles of
// two constants
CM_HD uint32_t cm_bam_code(uint32_t c) {
  if (c == '=') return 0u;
  const uint32_t u = (c | 0x20u) - 'a';
  if (u >= 26u) return 15u;  // (c | 0x20 is a lower-case letter exactly where c is a letter)
  return u < 16u ? (uint32_t)(0xFFF3FCFFB4FFD2E1ull >> (4u * u)) & 15u : (uint32_t)(0xFAF97F865Full >> (4u * (u - 16u))) & 15u;
}
// ... of the complement as the SAM line prints it on the - strand (sp_comp: anything but ACGT gives N)
CM_HD uint32_t cm_bam_comp_code(uint32_t c) {
  const uint32_t u = c & 0xDFu;
  return u == 'A' ? 8u : u == 'C' ? 4u : u == 'G' ? 2u : u == 'T' ? 1u : 15u;
}
// 33 off every byte of x, no borrow between bytes
CM_HD uint32_t cm_bam_sub33(uint32_t x) { return ((x | 0x80808080u) - 0x21212121u) ^ ((x ^ 0xDEDEDEDEu) & 0x80808080u); }

CM_HD uint32_t cm_bam_load32(const uint8_t *p) { uint32_t x; __builtin_memcpy(&x, p, 4); return x; }
CM_HD uint64_t cm_bam_load64(const uint8_t *p) { uint64_t x; __builtin_memcpy(&x, p, 8); return x; }
CM_HD void cm_bam_put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
CM_HD void cm_bam_put32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// what the group spreads: byte(t) is output byte t, word(t) the output bytes t .. t + 3 (little-endian), both below the part's length
struct CmBamBytes {  // name, CIGAR words, MD: as they are
  const uint8_t *s;
  CM_HD uint32_t byte(uint32_t t) const { return s[t]; }
  CM_HD uint32_t word(uint32_t t) const { return cm_bam_load32(s + t); }
};
struct CmBamQual {  // s[0 .. len) minus 33; !fwd: s[len - 1] first
  const uint8_t *s;
  uint32_t len;
  bool fwd;
  CM_HD uint32_t byte(uint32_t t) const { return ((uint32_t)(fwd ? s[t] : s[len - 1u - t]) - 33u) & 0xffu; }
  CM_HD uint32_t word(uint32_t t) const { return cm_bam_sub33(fwd ? cm_bam_load32(s + t) : __builtin_bswap32(cm_bam_load32(s + (len - 4u - t)))); }
};
struct CmBamSeq {  // the sl bases s[0 .. sl), two a byte; !fwd: reversed and complemented.  An odd sl leaves the last low nibble 0
  const uint8_t *s;
  uint32_t sl;
  bool fwd;
  CM_HD uint32_t code(uint32_t i) const { return i >= sl ? 0u : fwd ? cm_bam_code(s[i]) : cm_bam_comp_code(s[sl - 1u - i]); }
  CM_HD uint32_t byte(uint32_t t) const { return (code(2u * t) << 4) | code(2u * t + 1u); }
  CM_HD uint32_t word(uint32_t t) const {
    if (2u * t + 8u > sl) return byte(t) | (byte(t + 1u) << 8) | (byte(t + 2u) << 16) | (byte(t + 3u) << 24);
    // bases 2t .. 2t + 7 in one load; on the - strand they are s[sl - 8 - 2t .. sl - 1 - 2t], the last of them first
    const uint64_t x = fwd ? cm_bam_load64(s + 2u * t) : __builtin_bswap64(cm_bam_load64(s + (sl - 8u - 2u * t)));
    uint32_t w = 0;
    for (uint32_t k = 0; k < 8u; ++k) {
      const uint32_t c = (uint32_t)(x >> (8u * k)) & 0xffu;
      w |= (fwd ? cm_bam_code(c) : cm_bam_comp_code(c)) << (8u * (k >> 1) + ((k & 1u) ? 0u : 4u));
    }
    return w;
  }
};
// the group writes src's len bytes at dst: bytes up to dst's next 4-byte boundary, whole words, the last bytes (GT::G >= 4)
template <class GT, class S>
CM_HD void cm_bam_spread(const GT &g, uint8_t *dst, uint32_t len, const S &src) {
  uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
  if (head > len) head = len;
  if (g.t < head) dst[g.t] = (uint8_t)src.byte(g.t);
  const uint32_t words = (len - head) / 4u;
  for (uint32_t w = g.t; w < words; w += (uint32_t)GT::G) {
    const uint32_t t = head + 4u * w;
    *reinterpret_cast<uint32_t *>(dst + t) = src.word(t);
  }
  const uint32_t t = head + 4u * words + g.t;
  if (t < len) dst[t] = (uint8_t)src.byte(t);
}

// The record of r at dst (cm_bam_record_size bytes).  cg, md: its CIGAR words and MD bytes; name: the read's name (name_len <=
// CM_BAM_NAME_MAX: the caller refuses longer ones); bases, quals: the read as stored, of which the SAM line prints
// l_seq = cm_bam_seq_len bases -- the first l_seq on the + strand (r.strand != 0), else the reverse complement of the last l_seq of
// the first trim_len.  has_cb: the record ends with CB:Z and cb_len value bytes -- cb_plain: the 2-bit barcode bc_key as cb_len letters
// (Seed2Sequence); otherwise the value bytes are the caller's (a translated barcode) and this function writes the tag's head and
// its NUL.  Returns where the CB value stands.
template <class GT, class R>
CM_HD uint8_t *cm_bam_encode(const GT &g, uint8_t *dst, const R &r, const uint32_t *cg, const uint8_t *md, const uint8_t *name, uint32_t name_len,
                             const uint8_t *bases, const uint8_t *quals, bool has_cb, uint32_t cb_len, bool cb_plain, uint64_t bc_key) {
  const uint32_t sl = cm_bam_seq_len(cg, r.n_cigar, r.trim_len), nmb = cm_bam_nm_bytes(r.nm);
  const bool fwd = r.strand != 0;
  const uint32_t skip = fwd ? 0u : r.trim_len - sl;
  uint8_t *p_name = dst + 36, *p_cig = p_name + name_len + 1u, *p_seq = p_cig + 4u * r.n_cigar, *p_qual = p_seq + (sl + 1u) / 2u;
  uint8_t *p_nm = p_qual + sl, *p_md = p_nm + 3u + nmb, *p_cb = p_md + 3u + r.md_len + 1u;
  cm_bam_spread(g, p_name, name_len, CmBamBytes{name});
  cm_bam_spread(g, p_cig, 4u * r.n_cigar, CmBamBytes{reinterpret_cast<const uint8_t *>(cg)});
  cm_bam_spread(g, p_seq, (sl + 1u) / 2u, CmBamSeq{bases + skip, sl, fwd});
  cm_bam_spread(g, p_qual, sl, CmBamQual{quals + skip, sl, fwd});
  cm_bam_spread(g, p_md + 3, r.md_len, CmBamBytes{md});
  if (has_cb && cb_plain)
    for (uint32_t b = g.t; b < cb_len; b += (uint32_t)GT::G) p_cb[3u + b] = (uint8_t)"ACGT"[(bc_key >> ((cb_len - 1u - b) * 2u)) & 3u];
  if (g.t == 0) {
    const uint32_t rl = cm_bam_ref_len(cg, r.n_cigar);
    const uint64_t size = cm_bam_record_size(r, cg, name_len, has_cb, cb_len);
    cm_bam_put32(dst, (uint32_t)(size - 4u));
    cm_bam_put32(dst + 4, r.rid);
    cm_bam_put32(dst + 8, r.pos);
    dst[12] = (uint8_t)(name_len + 1u);
    dst[13] = (uint8_t)r.mapq;
    cm_bam_put16(dst + 14, cm_bam_reg2bin(r.pos, r.pos + (rl ? rl : 1u)));
    cm_bam_put16(dst + 16, r.n_cigar);
    cm_bam_put16(dst + 18, r.flag);
    cm_bam_put32(dst + 20, sl);
    cm_bam_put32(dst + 24, r.mrid < 0 ? 0xffffffffu : (uint32_t)r.mrid);
    cm_bam_put32(dst + 28, r.mrid < 0 ? 0xffffffffu : r.mpos);
    cm_bam_put32(dst + 32, (uint32_t)r.tlen);
    p_name[name_len] = 0;
    p_nm[0] = 'N'; p_nm[1] = 'M'; p_nm[2] = nmb == 1u ? 'C' : nmb == 2u ? 'S' : 'I';
    for (uint32_t b = 0; b < nmb; ++b) p_nm[3u + b] = (uint8_t)(r.nm >> (8u * b));
    p_md[0] = 'M'; p_md[1] = 'D'; p_md[2] = 'Z';
    p_md[3u + r.md_len] = 0;
    if (has_cb) {
      p_cb[0] = 'C'; p_cb[1] = 'B'; p_cb[2] = 'Z';
      p_cb[3u + cb_len] = 0;
    }
  }
  return p_cb + 3;
}
#endif
