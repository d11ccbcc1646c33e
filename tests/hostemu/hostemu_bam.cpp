// hostemu_bam.cpp -- TEST INFRASTRUCTURE.  The device's BAM record encoder (chromap_amd/csrc/cm_bam.h; cm_sam_post.hip: k_sp_len<true>,
// k_bam_format) on the host: the same size function, a sequential scan for the offsets, and the same group encoder run by emu_group.h's
// lanes -- 8, 16 or 64 of them, in ascending or descending order.  The encoder's lanes never wait for each other, so every lane runs
// through all records before the next one starts: whatever one lane's stores would owe to another's shows under one of the orders.
#include <stdint.h>
#include <string.h>

#include "../../chromap_amd/csrc/cm_bam.h"
#include "emu_group.h"

struct HostRec {  // the fields of cm_sam_post.hip's SpRec that the encoder reads, 12 32-bit words
  uint32_t rid, pos, mpos, nm;
  int32_t mrid, tlen;
  uint32_t flag, n_cigar, md_len, mapq, strand, trim_len;
};
struct Batch {
  uint64_t n;
  const HostRec *rec;
  const uint32_t *cigar;
  const uint64_t *cigar_off;  // in words
  const uint8_t *md;
  const uint64_t *md_off;
  const uint8_t *names;
  const uint64_t *name_off;
  const uint8_t *bases, *quals;
  const uint64_t *read_off;
  const uint64_t *bc;
  bool has_cb;
  uint32_t cb_len;
  uint8_t *out;
  const uint64_t *off;  // n + 1; a refused record has no bytes
};

template <int G>
static void encode_all(const Batch &b, bool reverse) {
  emu_run_group<G>([&](EmuGroup<G> &g) {
    for (uint64_t i = 0; i < b.n; ++i) {
      if (b.off[i + 1] == b.off[i]) continue;
      cm_bam_encode(g, b.out + b.off[i], b.rec[i], b.cigar + b.cigar_off[i], b.md + b.md_off[i], b.names + b.name_off[i],
                    (uint32_t)(b.name_off[i + 1] - b.name_off[i]), b.bases + b.read_off[i], b.quals + b.read_off[i], b.has_cb, b.cb_len, true,
                    b.has_cb ? b.bc[i] : 0);
    }
  }, reverse);
}

// The records of the batch back to back from out + start on.  off (n + 1 words) receives their offsets, from the size function; a read
// name of more than CM_BAM_NAME_MAX bytes is refused as the length kernel does it: no bytes, counted in *refused.  Returns the offset
// behind the last record; -1: cap is too small; -2: G is none of 8, 16, 64
extern "C" long hostemu_bam_encode(int G, int reverse, uint64_t n, const uint32_t *rec_words, const uint32_t *cigar, const uint64_t *cigar_off, const uint8_t *md,
                                   const uint64_t *md_off, const uint8_t *names, const uint64_t *name_off, const uint8_t *bases, const uint8_t *quals,
                                   const uint64_t *read_off, const uint64_t *bc, int has_cb, uint32_t cb_len, uint8_t *out, uint64_t start, uint64_t cap,
                                   uint64_t *off, uint64_t *refused) {
  static_assert(sizeof(HostRec) == 48, "twelve words");
  const HostRec *rec = reinterpret_cast<const HostRec *>(rec_words);
  *refused = 0;
  off[0] = start;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t name_len = (uint32_t)(name_off[i + 1] - name_off[i]);
    uint64_t sz = cm_bam_record_size(rec[i], cigar + cigar_off[i], name_len, has_cb != 0, cb_len);
    if (name_len > CM_BAM_NAME_MAX) { ++*refused; sz = 0; }
    off[i + 1] = off[i] + sz;
  }
  if (off[n] > cap) return -1;
  const Batch b = {n, rec, cigar, cigar_off, md, md_off, names, name_off, bases, quals, read_off, bc, has_cb != 0, cb_len, out, off};
  if (G == 8) encode_all<8>(b, reverse != 0);
  else if (G == 16) encode_all<16>(b, reverse != 0);
  else if (G == 64) encode_all<64>(b, reverse != 0);
  else return -2;
  return (long)off[n];
}
extern "C" uint32_t hostemu_bam_reg2bin(uint32_t beg, uint32_t end) { return cm_bam_reg2bin(beg, end); }
extern "C" uint32_t hostemu_bam_code(uint32_t c, int complemented) { return complemented ? cm_bam_comp_code(c) : cm_bam_code(c); }
extern "C" uint32_t hostemu_bam_sub33(uint32_t x) { return cm_bam_sub33(x); }
