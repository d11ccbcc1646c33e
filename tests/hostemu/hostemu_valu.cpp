// Host drivers for two per-read stage functions of chromap_amd/csrc/cm_stages.h, each against the function that defines its result:
//   cm_s3b_short (the short-list form of S3b: sorting network, one sweep)   against cm_s3b_candidates_lds (cm_s3b_core)
//   cm_pack_read_planes_w (the read's bit planes, four bytes at a time)    against cm_pack_read_planes_any
// and a driver for the MAPQ functions on plain arguments (hostemu_mapq_batch: what cmgpu_debug_mapq runs on the device), compared in
// tests/test_mapq_cpu.py with the model of tests/mapq_model.py and the oracle.
// Built into a library of its own by tests/hostemu_valu_lib.py for tests/test_s3b_short_cpu.py, tests/test_pack_planes_cpu.py and
// tests/test_mapq_cpu.py; tests/hostemu/mapq_san_main.cpp includes this file for its sanitizer build.
// Test infrastructure only.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/chromap_amd.h"
#include "../../chromap_amd/csrc/cm_mapq_tables.h"
#include "../../chromap_amd/csrc/cm_stages.h"

#define EMU_BLOCK 256  // the device kernel's block: slot i of lane t at S[i * 256 + t]

// n_reads reads (an even number: pairs), read r's lookup results at [mm_off[r], mm_off[r + 1]) of kind / val / ps, the occurrence table
// occ.  S3a sets the totals and the round, then every read with at most 16 hits goes through both forms of S3b, the lists' arrays
// prefilled alike.  Returns the number of reads compared, or -1 with *bad_read set.  tot_out / round2_out / ncand_out (n_reads each):
// what S3a and the defining form found, for the test's own coverage checks.
extern "C" long hostemu_s3b_short_check(uint32_t n_reads, const uint32_t *mm_off, const uint8_t *kind, const uint64_t *val, const uint32_t *ps,
                                        const uint64_t *occ, uint32_t n_occ, int e, int k, int w, int f0, int f1, int min_seeds,
                                        uint32_t *tot_out, uint8_t *round2_out, uint32_t *ncand_out, long *bad_read) {
  CmDev d;
  memset(&d, 0, sizeof d);
  d.p.e = e; d.p.k = k; d.p.w = w; d.p.f0 = f0; d.p.f1 = f1; d.p.min_seeds = min_seeds; d.p.single = 0;
  d.occ = occ; d.n_occ = n_occ;
  d.n_seq = 0x7fffffffu;
  d.n_pairs = n_reads / 2;
  std::vector<uint32_t> mm_cnt(n_reads), off(mm_off, mm_off + n_reads + 1), hit_tot(n_reads), hit_off(n_reads + 1), rep_cnt(n_reads), rep_len(n_reads);
  std::vector<uint8_t> round2(n_reads);
  for (uint32_t r = 0; r < n_reads; ++r) mm_cnt[r] = mm_off[r + 1] - mm_off[r];
  d.mm_cnt = mm_cnt.data(); d.mm_off = off.data();
  d.pr_kind = const_cast<uint8_t *>(kind); d.pr_val = const_cast<uint64_t *>(val); d.mm_ps = const_cast<uint32_t *>(ps);
  d.hit_tot = hit_tot.data(); d.hit_off = hit_off.data(); d.round2 = round2.data(); d.rep_cnt = rep_cnt.data(); d.rep_len = rep_len.data();
  for (uint32_t r = 0; r < n_reads; ++r) cm_s3a_count(d, r);
  uint64_t total = 0;
  for (uint32_t r = 0; r < n_reads; ++r) { hit_off[r] = (uint32_t)total; total += hit_tot[r]; }
  hit_off[n_reads] = (uint32_t)total;
  std::vector<uint64_t> hb[2];
  std::vector<uint8_t> hc[2];
  std::vector<uint32_t> npos[2], ncp[2], ncn[2];
  for (int v = 0; v < 2; ++v) {
    hb[v].assign(total + 1, 0xA5A5A5A5DEADBEEFull); hc[v].assign(total + 1, 0x5A);
    npos[v].assign(n_reads, 0xFFFFFFFFu); ncp[v].assign(n_reads, 0xFFFFFFFFu); ncn[v].assign(n_reads, 0xFFFFFFFFu);
  }
  std::vector<uint64_t> lds_h((size_t)CM_S3S_CAP * EMU_BLOCK);
  std::vector<uint8_t> lds_c((size_t)CM_S3S_CAP * EMU_BLOCK);
  long compared = 0;
  for (uint32_t r = 0; r < n_reads; ++r) {
    tot_out[r] = hit_tot[r]; round2_out[r] = round2[r]; ncand_out[r] = 0;
    if (hit_tot[r] > CM_S3S_CAP) continue;
    const uint32_t t = r % EMU_BLOCK;
    d.hbuf = hb[0].data(); d.hcnt = hc[0].data(); d.n_pos_hit = npos[0].data(); d.ncp = ncp[0].data(); d.ncn = ncn[0].data();
    std::fill(lds_h.begin(), lds_h.end(), 0x1111111111111111ull);
    cm_s3b_candidates_lds(d, r, lds_h.data() + t, lds_c.data() + t, CM_S3S_CAP, EMU_BLOCK);
    d.hbuf = hb[1].data(); d.hcnt = hc[1].data(); d.n_pos_hit = npos[1].data(); d.ncp = ncp[1].data(); d.ncn = ncn[1].data();
    std::fill(lds_h.begin(), lds_h.end(), 0x2222222222222222ull);
    cm_s3b_short<EMU_BLOCK>(d, r, lds_h.data(), t);
    // the lane's own column only
    for (size_t i = 0; i < lds_h.size(); ++i)
      if (i % EMU_BLOCK != t && lds_h[i] != 0x2222222222222222ull) { *bad_read = r; return -2; }
    ncand_out[r] = ncp[0][r] + ncn[0][r];
    ++compared;
  }
  for (uint32_t r = 0; r < n_reads; ++r) {
    if (hit_tot[r] > CM_S3S_CAP) continue;
    bool ok = npos[0][r] == npos[1][r] && ncp[0][r] == ncp[1][r] && ncn[0][r] == ncn[1][r];
    for (uint32_t i = hit_off[r]; ok && i < hit_off[r + 1]; ++i) ok = hb[0][i] == hb[1][i] && hc[0][i] == hc[1][i];
    if (!ok) { *bad_read = r; return -1; }
  }
  return compared;
}

// Every length 1 .. max_len (at most 256) at every start alignment 0 .. 7, the bases taken from `pool` at a moving offset
// (pool_len >= max_len + 64: max_len + 48 bytes are copied per case); the bytes around the read are pool bytes too, so nothing beyond the length may show.  Two batches per case: W = the
// read's own number of words, where both forms define all 6 W words, and W one larger (a shorter read of a longer batch), where the
// words the defining form writes are compared.  Returns the number of cases, or -1 with *bad_len / *bad_align set.
extern "C" long hostemu_pack_planes_check(const uint8_t *pool, uint32_t pool_len, uint32_t max_len, uint32_t *bad_len, uint32_t *bad_align) {
  if (max_len > 256 || pool_len < max_len + 64) return -3;
  long cases = 0;
  uint32_t at = 0;
  std::vector<uint64_t> store((max_len + 64) / 8 + 2);
  uint8_t *buf = reinterpret_cast<uint8_t *>(store.data());
  for (uint32_t L = 1; L <= max_len; ++L) {
    for (uint32_t al = 0; al < 8; ++al) {
      at = (at + 37) % (pool_len - (max_len + 48));
      memcpy(buf, pool + at, max_len + 48);  // the read: L bytes from buf + 8 + al
      const uint32_t nw = (L + 31) >> 5;
      for (uint32_t W = nw; W <= nw + 1 && W <= 8; ++W) {
        CmDev d;
        memset(&d, 0, sizeof d);
        uint32_t ro[2] = {8 + al, 8 + al + L}, rlen[2] = {L, 0};
        d.rb0 = buf; d.rb1 = buf; d.ro0 = ro; d.ro1 = ro; d.rlen = rlen; d.n_pairs = 1;
        d.read_pl_w = W;
        const uint32_t stride = cm_read_pl_stride(W);
        std::vector<uint32_t> pa(2 * stride + 4, 0xC3C3C3C3u), pb(2 * stride + 4, 0xC3C3C3C3u);
        d.read_pl = pa.data(); cm_pack_read_planes_any(d, 0);
        d.read_pl = pb.data(); cm_pack_read_planes(d, 0);
        bool ok = true;
        for (uint32_t o = 0; o < 6; ++o)
          for (uint32_t wd = 0; wd < nw; ++wd) ok = ok && pa[o * W + wd] == pb[o * W + wd];
        for (uint32_t i = stride; i < pb.size(); ++i) ok = ok && pb[i] == 0xC3C3C3C3u;  // nothing beyond the read's own planes
        if (!ok) { *bad_len = L; *bad_align = al; return -1; }
        ++cases;
      }
    }
  }
  return cases;
}

// The MAPQ functions on their own (the device hook cmgpu_debug_mapq, include/chromap_amd_debug.h, on the host): n cases as the same two
// column-major matrices -- reads: 9 columns of 2 n values (num_errors, alignment_length, read_length, min_err, second_err, n_best,
// n_second, rep_len, strand_ncand), pairs: 6 columns of n values (max_diff, min_sum, second_sum, n_best, n_second, force_mapq) -- with
// the tables of cm_build_len_coef / cm_build_nsec_break.  kind: 0 cm_mapq_single, 1 cm_mapq_single_split, 2 cm_mapq_paired,
// 3 cm_mapq_paired_split.  coef_out (65536) / brk_out (capacity brk_cap) / n_brk_out: the tables themselves, or NULL.
extern "C" int hostemu_mapq_batch(int kind, int e, uint64_t n, const int32_t *reads, const int32_t *pairs, uint8_t *out, double *coef_out,
                                  uint32_t *brk_out, uint32_t brk_cap, uint32_t *n_brk_out) {
  static std::vector<double> coef;
  static std::vector<uint32_t> brk;
  if (coef.empty()) { cm_build_len_coef(coef); cm_build_nsec_break(brk); }
  if (coef_out) memcpy(coef_out, coef.data(), coef.size() * 8);
  if (n_brk_out) *n_brk_out = (uint32_t)brk.size();
  if (brk_out) {
    if (brk_cap < brk.size()) return -1;
    memcpy(brk_out, brk.data(), brk.size() * 4);
  }
  if (kind < 0 || kind > 3 || n > (1ull << 30)) return -1;
  CmDev d;
  memset(&d, 0, sizeof d);
  d.mq.len_coef = coef.data(); d.mq.nsec_break = brk.data(); d.mq.n_break = (int)brk.size();
  d.p.e = e;
  d.n_pairs = (uint32_t)n;
  const size_t n2 = 2 * (size_t)n;
  int32_t *col = const_cast<int32_t *>(reads);
  d.min_err = col + 3 * n2; d.second_err = col + 4 * n2; d.n_best = col + 5 * n2; d.n_second = col + 6 * n2;
  d.rep_len = reinterpret_cast<uint32_t *>(col + 7 * n2);
  const int32_t *err = reads, *al = reads + n2, *len = reads + 2 * n2, *nc = reads + 8 * n2;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t r1 = 2 * (uint32_t)i, r2 = r1 + 1;
    uint8_t q;
    if (kind == 0) {
      q = cm_mapq_single(d, err[r1], (uint16_t)al[r1], len[r1], pairs[i], d.second_err[r1], d.n_best[r1], d.n_second[r1], d.rep_len[r1]);
    } else if (kind == 1) {
      q = cm_mapq_single_split(d, err[r1], (uint16_t)al[r1], len[r1], pairs[i], d.second_err[r1], d.n_best[r1], d.n_second[r1], d.rep_len[r1],
                               (uint32_t)nc[r1]);
    } else if (kind == 2) {
      CmPe pe;
      pe.min_sum = pairs[n + i]; pe.second_sum = pairs[2 * n + i]; pe.n_best = pairs[3 * n + i]; pe.n_second = pairs[4 * n + i];
      pe.f_dir = pe.f_i1 = pe.f_i2 = 0;
      q = cm_mapq_paired(d, (uint32_t)i, err[r1], err[r2], (uint16_t)al[r1], (uint16_t)al[r2], len[r1], len[r2], pairs[5 * n + i], pe);
    } else {
      q = cm_mapq_paired_split(d, (uint32_t)i, err[r1], err[r2], (uint16_t)al[r1], (uint16_t)al[r2], len[r1], len[r2], (uint32_t)nc[r1],
                               (uint32_t)nc[r2]);
    }
    out[i] = q;
  }
  return 0;
}
