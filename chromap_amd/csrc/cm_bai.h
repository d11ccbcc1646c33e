// cm_bai.h -- the BAM index (.bai; SAM spec 5.2) of a chain of BAM alignment records that cm_bgzf_out.hip has compressed: what a
// record and the finished index need, written so that the device (cm_tabix.hip) and a host without one (tests/hostemu/hostemu_bai.cpp)
// run the same functions.  The binning scheme, the 16 kb linear index, the chunk rules and the pseudo-bin are the tabix index's
// (cm_tabix.h): the virtual offsets (cm_tbx_voff), the raw chunks' merge (cm_tbx_chunk_flag, cm_tbx_chunk_emit) and the way a shared
// word is written (`A::min64`) are taken from there.  What differs is where the keys come from -- fields of binary records that
// begin at any byte offset, not columns of text lines -- and that a reference is a number the record holds, below the header's
// n_ref, not a run of lines with one name: the per-reference table is indexed by refID, and a reference without records is empty.
//  1. per record i, which lies at starts[i] .. starts[i + 1]: its fields read and checked against its neighbours in the chain and
//     in the file (cm_bai_rec_parse) -- reference, [pos, end) with end = pos + max(1, reference length of the CIGAR), flag bit 4.
//     The first offending record: one 64-bit minimum of record << 3 | cause.
//  2. per record, once no record offends: the head flag of (reference, bin), what its reference has to know (cm_bai_rec_flags_core);
//     after a scan of the flags, the raw chunks and the linear index's minima (cm_bai_rec_emit).
//  3. per raw chunk, sorted by (reference, bin) with a stable sort: cm_tabix.h's stage 3.
//  4. the payload, on the host (cm_bai_serialize): a plain file, not BGZF.
// Sparse bins are not folded into their parents (htslib's compress_binning): the index is valid, and larger than samtools' own.
// With CmBaiArrays::csi_depth 1 .. 6 the same stages make a CSI index's keys (cm_tabix.h: depth levels, limit 2^(14 + 3 * depth) and
// 0xffffffff at depth 6, keys reference << 20 | bin); 0 is the .bai's scheme.  pos + reference length is a 64-bit sum before it is
// compared with the limit: a record at pos 2^31 - 1 does not wrap.
#ifndef CM_BAI_H_
#define CM_BAI_H_
#include "cm_bam.h"
#include "cm_tabix.h"

#define CM_BAI_MAX_RECORDS 0xfffffffeull
// why a chain of records cannot be indexed (the low three bits of the error word)
#define CM_BAI_E_MALFORMED 1u  // the record does not end where the next one starts, or is too short for its name and CIGAR
#define CM_BAI_E_NOREF 2u      // refID is no reference of the header (an unmapped record's -1 among them)
#define CM_BAI_E_UNSORTED 3u   // a smaller refID than the record before, or the same and a smaller pos
#define CM_BAI_E_RANGE 4u      // an end beyond 2^29 (beyond the depth's limit for a CSI)

struct CmBaiRef {  // one reference of the header
  uint64_t vbeg, vend;                     // virtual offsets of its first record's start and its last record's end
  unsigned long long n_mapped, n_unmapped; // its records without and with flag bit 4
  uint32_t n_intv, pad;                    // 0: no record
};
struct CmBaiArrays {
  CmTbxText t;              // p: the records' bytes; n: how many
  uint64_t n_rec;
  const uint64_t *starts;   // n_rec + 1: where every record starts, and n
  uint32_t n_ref;
  uint32_t *beg, *end;      // per record; end > beg
  uint32_t *tid;            // per record: its reference
  uint32_t *cidx;           // per record: 1 where (reference, bin) differs from the record's before; after the scan 1 + raw chunk
  unsigned long long *err;  // the smallest record << 3 | cause
  CmBaiRef *ref;            // n_ref
  const uint64_t *lin_off;  // per reference: where its windows begin in lin
  unsigned long long *lin;  // per window of 16 kb: the smallest virtual offset of a record that overlaps it
  uint64_t *ckey, *cbeg, *cend;  // per raw chunk, in file order
  uint32_t *cval;                // per raw chunk: its own number (the sort carries it)
  uint32_t csi_depth;            // 0: the .bai's scheme; 1 .. 6: a CSI of that depth
};

CM_HD uint32_t cm_bai_load16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// ---- 1. per record: tid, beg, end; the record's error word, where it has one
// (Nothing is read outside [0, n): every load is behind the comparison that shows it lies inside.)
template <class A>
CM_HD void cm_bai_rec_parse(const CmBaiArrays &d, uint64_t i) {
  const uint8_t *p = d.t.p;
  const uint64_t n = d.t.n, s = d.starts[i], e = d.starts[i + 1];
  uint32_t tid = 0, beg = 0, end = 1, cause = 0;
  if ((i == 0 && s != 0) || (i + 1 == d.n_rec && e != n) || e > n || s > e || e - s < 36u) {
    cause = CM_BAI_E_MALFORMED;
  } else {
    const uint32_t block_size = cm_bam_load32(p + s), l_name = p[s + 12], n_cigar = cm_bai_load16(p + s + 16);
    if (4ull + block_size != e - s || block_size < 32u + l_name + 4u * n_cigar) {
      cause = CM_BAI_E_MALFORMED;
    } else {
      const int32_t rid = (int32_t)cm_bam_load32(p + s + 4), pos = (int32_t)cm_bam_load32(p + s + 8);
      uint64_t rl = 0;  // (65535 operations of up to 2^28 - 1 bases)
      for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t w = cm_bam_load32(p + s + 36u + l_name + 4u * k);
        rl += cm_bam_ref_len(&w, 1);
      }
      if (rid < 0 || (uint32_t)rid >= d.n_ref) {
        cause = CM_BAI_E_NOREF;
      } else {
        // the record before, where its fixed fields lie inside the bytes (where they do not, that record is the first offender)
        if (i > 0 && d.starts[i - 1] <= s && s - d.starts[i - 1] >= 12u) {
          const uint64_t sp = d.starts[i - 1];
          const int32_t prid = (int32_t)cm_bam_load32(p + sp + 4), ppos = (int32_t)cm_bam_load32(p + sp + 8);
          if (rid < prid || (rid == prid && pos < ppos)) cause = CM_BAI_E_UNSORTED;
        }
        const uint64_t end64 = (uint64_t)(pos < 0 ? 0 : pos) + (rl ? rl : 1u);
        if (!cause && (pos < 0 || end64 > cm_csi_max_end(cm_tbx_depth_of(d.csi_depth)))) cause = CM_BAI_E_RANGE;
        if (!cause || cause == CM_BAI_E_UNSORTED) tid = (uint32_t)rid;
        if (!cause) { beg = (uint32_t)pos; end = (uint32_t)end64; }
      }
    }
  }
  if (cause) A::min64(d.err, (unsigned long long)i << 3 | cause);
  d.tid[i] = tid;
  d.beg[i] = beg;
  d.end[i] = end;
}

// ---- 2. record i of a chain without offenders: the head flag of (reference, bin), its reference's first and last virtual offset.
// Returns the windows the record asks of its reference's linear index; *ref_of its reference, *unmapped its flag bit 4 (the caller
// raises CmBaiRef::n_intv and the two counts: a wave does it for all its lanes)
CM_HD uint32_t cm_bai_rec_flags_core(const CmBaiArrays &d, uint64_t i, uint32_t *ref_of, uint32_t *unmapped) {
  const uint32_t t = d.tid[i], beg = d.beg[i], end = d.end[i];
  const bool head = i == 0 || d.tid[i - 1] != t;
  const bool tail = i + 1 == d.n_rec || d.tid[i + 1] != t;
  const uint32_t depth = cm_tbx_depth_of(d.csi_depth);
  d.cidx[i] = head || cm_csi_reg2bin(beg, end, depth) != cm_csi_reg2bin(d.beg[i - 1], d.end[i - 1], depth) ? 1u : 0u;
  CmBaiRef &r = d.ref[t];
  if (head) r.vbeg = cm_tbx_voff(d.t, d.starts[i]);
  if (tail) r.vend = cm_tbx_voff(d.t, d.starts[i + 1]);
  *ref_of = t;
  *unmapped = (cm_bai_load16(d.t.p + d.starts[i] + 18) >> 2) & 1u;
  return ((end - 1u) >> 14) + 1u;
}
// record i, cidx scanned: the raw chunk it begins and the one it ends, and its start's virtual offset as a candidate for the windows
// it overlaps.  (The first window is left out where the record before lies in it too: that record's offset is the smaller one.)
template <class A>
CM_HD void cm_bai_rec_emit(const CmBaiArrays &d, uint64_t i) {
  const uint32_t t = d.tid[i], ci = d.cidx[i] - 1u, beg = d.beg[i], end = d.end[i];
  const bool head = i == 0 || d.tid[i - 1] != t;
  const uint64_t vs = cm_tbx_voff(d.t, d.starts[i]);
  if (i == 0 || d.cidx[i - 1] != d.cidx[i]) {
    d.ckey[ci] = (uint64_t)t << cm_tbx_key_shift_of(d.csi_depth) | cm_csi_reg2bin(beg, end, cm_tbx_depth_of(d.csi_depth));
    d.cbeg[ci] = vs;
    d.cval[ci] = ci;
  }
  if (i + 1 == d.n_rec || d.cidx[i + 1] != d.cidx[i]) d.cend[ci] = cm_tbx_voff(d.t, d.starts[i + 1]);
  uint32_t w = beg >> 14;
  const uint32_t w1 = (end - 1u) >> 14;
  if (!head && d.beg[i - 1] >> 14 == w) ++w;
  unsigned long long *lin = d.lin + d.lin_off[t];
  for (; w <= w1; ++w) A::min64(lin + w, vs);
}

// ---- 4. the payload (host).  ch: the merged chunks in (reference, bin, file) order; lin: all references' windows, back-filled
static inline void cm_bai_serialize(const CmBaiRef *ref, uint32_t n_ref, const CmTbxChunk *ch, uint64_t n_ch, const uint64_t *lin, const uint64_t *lin_off,
                                    std::vector<uint8_t> &o) {
  o.clear();
  o.reserve(16 + (size_t)n_ref * 48 + n_ch * 24 + (n_ref ? lin_off[n_ref] * 8 : 0));
  const uint8_t magic[4] = {'B', 'A', 'I', 1};
  o.insert(o.end(), magic, magic + 4);
  cm_tbx_put(o, n_ref, 4);
  uint64_t at = 0;
  for (uint32_t r = 0; r < n_ref; ++r) {
    if (ref[r].n_intv == 0) {  // no record: no bin, not the pseudo-bin either, no window
      cm_tbx_put(o, 0, 8);
      continue;
    }
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
    cm_tbx_put(o, ref[r].n_mapped, 8);
    cm_tbx_put(o, ref[r].n_unmapped, 8);
    cm_tbx_put(o, ref[r].n_intv, 4);
    for (uint64_t w = lin_off[r]; w < lin_off[r + 1]; ++w) cm_tbx_put(o, lin[w], 8);
  }
  cm_tbx_put(o, 0, 8);  // n_no_coor: no unmapped record is written
}
// the message for an error word
static inline const char *cm_bai_cause(uint32_t cause) {
  return cause == CM_BAI_E_MALFORMED ? "is malformed: it does not end where the next one starts, or is shorter than its name and CIGAR"
       : cause == CM_BAI_E_NOREF    ? "has no reference of the header (a refID below 0 or not below n_ref): records without a position are not indexed"
       : cause == CM_BAI_E_UNSORTED ? "lies before the record ahead of it: the records are not sorted by reference and position"
                                    : "ends beyond 2^29, the limit of the BAI format (samtools index -c or --output-csi builds a .csi index for such a file)";
}
// ... for a CSI of the given depth
static inline std::string cm_csi_bai_cause(uint32_t cause, uint32_t depth) {
  if (cause != CM_BAI_E_RANGE) return cm_bai_cause(cause);
  return "ends beyond " + cm_csi_limit_words(depth) + ", the limit of a CSI index of depth " + std::to_string(depth);
}
#endif
