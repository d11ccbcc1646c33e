// Host drivers for the stage functions of the front end's planes route (chromap_amd/csrc/cm_stages.h; k_prep_mm's planes instance: a
// read of at most 64 bases is converted to bit planes once, for the trim, the minimizer pass and the verification's planes), each against
// the function that defines its result:
//   cm_read_planes64 + cm_finish_read_planes             against cm_pack_read_planes_any (bytes, cm_c2u) and cm_pack_read_planes_w
//   cm_s0_prep_ptr with the pair's planes (cm_trim_planes64)   against cm_s0_prep_ptr on bytes (and, from the test, the oracle's trim)
//   cm_minimizers_w7_planes                               against cm_minimizers_w7 on bytes and the state machine
// Built into a library of its own by tests/hostemu_pack_once_lib.py for tests/test_pack_once_cpu.py, and into a stand-alone program
// by tests/hostemu/pack_once_san_main.cpp.  Test infrastructure only.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/chromap_amd.h"
#include "../../chromap_amd/csrc/cm_mapq_tables.h"
#include "../../chromap_amd/csrc/cm_stages.h"

// Every length 1 .. 64 at every start alignment 0 .. 15 and every trimmed length L = 0 .. len, the bases taken from `pool` at a moving
// offset (pool_len >= 256); the bytes around the read are pool bytes too, so nothing beyond the length may show.  Batches of W = 1
// (reads of up to 32 bases) and W = 2 words per plane.  Against the byte definition on the words it defines, against the
// four-bytes-at-a-time form on every word of the read's stride; nothing written beyond the stride, nothing at all for L = 0.
// Returns the number of cases, or -1 with bad[0..3] = len, alignment, L, W.
extern "C" long hostemu_po_planes_check(const uint8_t *pool, uint32_t pool_len, uint32_t *bad) {
  if (pool_len < 256) return -3;
  long cases = 0;
  uint32_t at = 0;
  std::vector<uint64_t> store(20);
  uint8_t *buf = reinterpret_cast<uint8_t *>(store.data());
  for (uint32_t len = 1; len <= 64; ++len)
    for (uint32_t al = 0; al < 16; ++al) {
      at = (at + 37) % (pool_len - 128);
      memcpy(buf, pool + at, 128);  // the read: len bytes from buf + 16 + al
      uint64_t p0, p1, pn, pu;
      cm_read_planes64(buf + 16 + al, len, &p0, &p1, &pn, &pu);
      for (uint32_t i = 0; i < len; ++i) {  // pu: everything but upper-case A C G T
        const uint8_t ch = buf[16 + al + i];
        const bool up = ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T';
        if ((((pu >> i) & 1u) != 0) == up) { bad[0] = len; bad[1] = al; bad[2] = i; bad[3] = 0; return -2; }
      }
      for (uint32_t L = 0; L <= len; ++L)
        for (uint32_t W = (len + 31) / 32; W <= 2; ++W) {
          CmDev d;
          memset(&d, 0, sizeof d);
          uint32_t ro[2] = {16 + al, 16 + al + len}, rlen[2] = {L, 0};
          d.rb0 = buf; d.rb1 = buf; d.ro0 = ro; d.ro1 = ro; d.rlen = rlen; d.n_pairs = 1;
          d.read_pl_w = W;
          const uint32_t stride = cm_read_pl_stride(W), nw = (L + 31) >> 5;
          std::vector<uint32_t> pa(2 * stride + 4, 0xC3C3C3C3u), pb(pa), pc(pa);
          d.read_pl = pa.data(); cm_pack_read_planes_any(d, 0);
          d.read_pl = pb.data(); cm_pack_read_planes(d, 0);
          d.read_pl = pc.data(); cm_finish_read_planes(d, 0, p0, p1, pn, L);
          bool ok = true;
          for (uint32_t o = 0; o < 6; ++o)
            for (uint32_t wd = 0; wd < nw; ++wd) ok = ok && pa[o * W + wd] == pc[o * W + wd];
          for (uint32_t i = 0; i < pc.size(); ++i) ok = ok && pb[i] == pc[i];  // (beyond the stride, and everywhere for L = 0: the fill)
          if (!ok) { bad[0] = len; bad[1] = al; bad[2] = L; bad[3] = W; return -1; }
          ++cases;
        }
    }
  return cases;
}

// S0 alone (length filter + adapter trimming) as the planes instance of k_prep_mm runs it: both reads converted by cm_read_planes64,
// cm_s0_prep_ptr with the planes.  A pair with a read of more than 64 bases goes without planes (such a batch does not run that
// instance).  rlen[2 * pair], rlen[2 * pair + 1]; *n_planes: the pairs whose planes the fast path accepted (upper-case A/C/G/T only).
extern "C" int hostemu_po_trim(const cmgpu_params *params, const cmgpu_batch *in, uint32_t *rlen, uint32_t *n_planes) {
  CmDev d;
  memset(&d, 0, sizeof(d));
  d.p.min_read_len = params->min_read_length;
  d.p.trim = params->trim_adapters;
  d.rb0 = (const uint8_t *)in->read1_bases; d.rb1 = (const uint8_t *)in->read2_bases;
  d.ro0 = in->read1_offsets; d.ro1 = in->read2_offsets;
  d.rlen = rlen;
  *n_planes = 0;
  for (uint32_t i = 0; i < in->n_pairs; ++i) {
    const uint32_t raw[2] = {d.ro0[i + 1] - d.ro0[i], d.ro1[i + 1] - d.ro1[i]};
    const uint8_t *s[2] = {d.rb0 + d.ro0[i], d.rb1 + d.ro1[i]};
    if (raw[0] > 64 || raw[1] > 64) { cm_s0_prep_ptr(d, i, s[0], s[1]); continue; }
    CmPairPlanes pp;
    for (int m = 0; m < 2; ++m) {
      uint64_t pn, pu;
      cm_read_planes64(s[m], raw[m], &pp.p0[m], &pp.p1[m], &pn, &pu);
      pp.upper[m] = (pu & cm_mask64(raw[m])) == 0;
    }
    *n_planes += pp.upper[0] && pp.upper[1];
    cm_s0_prep_ptr(d, i, s[0], s[1], &pp);
  }
  return 0;
}

// one read's minimizers (w = 7).  route 0: from its planes, as the planes instance of k_prep_mm takes them (a base outside ACGT
// sends the read to the state machine); 1: cm_minimizers_w7 on bytes; 2: the state machine.  The read is copied to byte alignment
// `align` (0 .. 15) first.
extern "C" int hostemu_po_minimizers(const uint8_t *seq, uint32_t len, int k, int route, uint32_t align, uint64_t *out_hash, uint32_t *out_ps,
                                     uint32_t cap) {
  std::vector<uint64_t> store((len + 16 + 15) / 8 + 2);
  uint8_t *rd = reinterpret_cast<uint8_t *>(store.data()) + (align & 15u);
  memcpy(rd, seq, len);
  auto put = [&](uint32_t n, uint64_t h, uint32_t p) { if (n < cap) { out_hash[n] = h; out_ps[n] = p; } };
  if (route == 1) return (int)cm_minimizers_w7(rd, len, k, put);
  if (route == 2) return (int)cm_minimizers_window_e<7>(rd, len, k, put);
  if (len > 64) return -1;
  uint64_t p0, p1, pn, pu;
  cm_read_planes64(rd, len, &p0, &p1, &pn, &pu);
  return (int)cm_minimizers_w7_planes(p0, p1, (pn & cm_mask64(len)) != 0, rd, len, k, put);
}
