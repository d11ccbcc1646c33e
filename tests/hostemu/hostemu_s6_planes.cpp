// Host drivers for S6's mismatch count on bit planes (chromap_amd/csrc/cm_stages.h: cm_hamming_diag_planes, and cm_ref_start_end, which
// takes it for "plain" reads -- upper-case A/C/G/T only, at most 64 bases) against the byte count it stands for (cm_hamming_diag on the
// bytes the planes were packed from).  Built into a library of its own by tests/hostemu_s6_planes_lib.py for tests/test_s6_planes_cpu.py,
// and into a stand-alone program by tests/hostemu/s6_planes_san_main.cpp.  Test infrastructure only.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/chromap_amd.h"
#include "../../chromap_amd/csrc/cm_mapq_tables.h"
#include "../../chromap_amd/csrc/cm_stages.h"

namespace {
struct Rng {  // xorshift64*: the cases are the same in the library and in the stand-alone program
  uint64_t s;
  uint32_t next(uint32_t n) { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (uint32_t)(((s * 0x2545F4914F6CDD1Dull) >> 33) % n); }
};
const char BASES[] = "ACGT";
uint8_t comp(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }
uint8_t other_base(uint8_t c, uint32_t k) {  // an upper-case base that differs from the letter c in either case
  const uint8_t u = c & 0xDFu;
  uint32_t i = 0;
  while (i < 4 && (uint8_t)BASES[i] != u) ++i;
  return (uint8_t)BASES[(i + 1 + k % 3) & 3];
}
// reference bytes -> plane records of the whole buffer, as k_pack_ref writes them (CM_PL_LEAD zero records in front, four behind)
std::vector<CmPlRec> pack_ref(const std::vector<uint8_t> &ref) {
  const size_t words = (ref.size() + 31) / 32 + 4;
  std::vector<CmPlRec> pl(words + CM_PL_LEAD, CmPlRec{0u, 0u, 0u, 0u});
  for (size_t w = 0; 32 * w < ref.size(); ++w) {
    uint8_t b[48] = {0};
    const size_t n = ref.size() - 32 * w < 32 ? ref.size() - 32 * w : 32;
    memcpy(b, ref.data() + 32 * w, n);
    CmPlRec &r = pl[w + CM_PL_LEAD];
    cm_pack_planes32(b, 32, &r.p0, &r.p1, &r.pn, &r.pc);
  }
  return pl;
}
// a read's planes the way k_prep_mm's planes instance leaves them: cm_read_planes64 on the raw bytes, cm_finish_read_planes at the
// trimmed length; returns the kernel's "plain" flag
uint32_t pack_read(CmDev &d, uint32_t r, const uint8_t *raw, uint32_t raw_len, uint32_t L) {
  uint64_t p0, p1, pn, pu;
  cm_read_planes64(raw, raw_len, &p0, &p1, &pn, &pu);
  cm_finish_read_planes(d, r, p0, p1, pn, L);
  return (pu & cm_mask64(raw_len)) == 0 ? 1u : 0u;
}
}  // namespace

// One case of the count.  The window's first base lies at g with g & 31 = sh; a chromosome starts at byte 64 of the reference buffer.
//   mis: 0 none, 1 the first base, 2 the last base, 3 first + middle + last, 4 every base
//   ref_kind: 0 upper-case letters; 1 lower-case letters in the window (one of them under a substituted base when mis != 0);
//             2 N and n in the window; 3 the window runs two bases into the zero padding behind the chromosome; 4 all of these
//   extra: bases of the raw read beyond the trimmed length L (the - strand's text is the reverse complement of the first L)
// out[0] = cm_hamming_diag on bytes, out[1] / out[2] = cm_hamming_diag_planes with one (L <= 32 only, else a copy of out[2]) / two words
// per read plane, out[3] = the mismatches the case was built with (counted while building), out[4] = the read's plain flag.
// Returns 0, or a negative number for parameters outside the sweep.
extern "C" int hostemu_s6p_case(uint32_t L, uint32_t sh, int strand, int mis, int ref_kind, uint32_t extra, uint64_t seed, int32_t *out) {
  if (L < 1 || L > 64 || sh > 31 || mis < 0 || mis > 4 || ref_kind < 0 || ref_kind > 4 || L + extra > 64) return -1;
  Rng rng{seed * 0x9E3779B97F4A7C15ull + 0x1234567ull + L * 131u + sh * 7u + (uint32_t)strand};
  const uint64_t g = 64 + 96 + sh;
  const bool pad = ref_kind == 3 || ref_kind == 4;
  const uint32_t over = pad ? (L > 2 ? 2u : 1u) : 0u;
  const uint32_t rl = (uint32_t)(g - 64) + L - over + (pad ? 0u : 40u);
  std::vector<uint8_t> ref(64 + rl + 64 + 16, 0);
  for (uint32_t i = 0; i < rl; ++i) ref[64 + i] = (uint8_t)BASES[rng.next(4)];
  // the text: the window in upper case (anything for the bases over the end), then the substitutions
  std::vector<uint8_t> text(L);
  for (uint32_t i = 0; i < L; ++i) text[i] = i < L - over ? ref[g + i] : (uint8_t)BASES[rng.next(4)];
  std::vector<uint8_t> sub(L, 0);
  if (mis == 1 || mis == 3) sub[0] = 1;
  if (mis == 2 || mis == 3) sub[L - 1] = 1;
  if (mis == 3) sub[L / 2] = 1;
  if (mis == 4) sub.assign(L, 1);
  for (uint32_t i = 0; i < L; ++i) if (sub[i] && i < L - over) text[i] = other_base(text[i], rng.next(3));
  // the window's special bytes
  std::vector<uint8_t> special(L, 0);
  if (ref_kind == 1 || ref_kind == 4) {
    ref[g] |= 0x20; special[0] = 1;  // (under the first base: a substituted one when mis is 1, 3 or 4)
    if (L > 5) { ref[g + 5] |= 0x20; special[5] = 1; }
  }
  if (ref_kind == 2 || ref_kind == 4) {
    if (L > 3) { ref[g + 3] = 'N'; special[3] = 1; }
    if (L > 9 + over) { ref[g + L - 1 - over] = 'n'; special[L - 1 - over] = 1; }
    if (L <= 3) { ref[g + L - 1 - over] = 'N'; special[L - 1 - over] = 1; }
  }
  int built = 0;
  for (uint32_t i = 0; i < L; ++i) built += (sub[i] || special[i] || i >= L - over) ? 1 : 0;
  // the raw read: the text (its reverse complement on the - strand), then `extra` more bases
  std::vector<uint8_t> raw(L + extra + 32, 0);
  for (uint32_t i = 0; i < L; ++i) raw[i] = strand ? comp(text[L - 1 - i]) : text[i];
  for (uint32_t i = 0; i < extra; ++i) raw[L + i] = (uint8_t)BASES[rng.next(4)];
  const std::vector<CmPlRec> pl = pack_ref(ref);
  out[0] = cm_hamming_diag(ref.data() + g, raw.data(), (int)L, strand != 0, 0, (int)L);
  for (uint32_t W = 1; W <= 2; ++W) {
    if (W == 1 && L + extra > 32) { continue; }
    CmDev d;
    memset(&d, 0, sizeof d);
    std::vector<uint32_t> planes(cm_read_pl_stride(W) + 4, 0xC3C3C3C3u);
    d.read_pl = planes.data(); d.read_pl_w = W;
    out[4] = (int32_t)pack_read(d, 0, raw.data(), L + extra, L);
    out[W] = cm_hamming_diag_planes(pl.data() + CM_PL_LEAD, g, cm_read_pl_of(d, 0) + (strand ? 3 * W : 0), W, (int)L);
  }
  if (L + extra > 32) out[1] = out[2];
  out[3] = built;
  return 0;
}

// cm_ref_start_end with "s6_planes" on and off for one read of a one-read batch, placed `pos` bases into a chromosome of 300 bases:
//   kind 0: 50 plain bases, two substitutions;  1: the same with one base deleted from the read (the count fails, the byte traceback runs);
//   2: 50 bases with an N;  3: 50 bases with a lower-case base;  4: 65 plain bases;  5: kind 0 in the chromosome's last bases (the
//   window clamp);  6: kind 0 at the chromosome's first base
// For kinds 2-4 the read's planes are filled with a pattern that is no packing of the read: equal results show the byte route.
// out[0..2] = the span with the option on (rid, start, end), out[3..5] = with it off, out[6] = the read's flag as the front end sets it,
// out[7] = the edit distance handed in, out[8] = pos.
extern "C" int hostemu_s6p_dispatch(int kind, int strand, uint64_t seed, uint32_t *out) {
  if (kind < 0 || kind > 6) return -1;
  Rng rng{seed * 0x9E3779B97F4A7C15ull + 77u + (uint32_t)kind * 1315423911u + (uint32_t)strand};
  const uint32_t rl = 300, e = 4, L = kind == 4 ? 65u : 50u;
  const uint32_t pos = kind == 5 ? rl - L : kind == 6 ? 0u : 100u + rng.next(32);
  std::vector<uint8_t> ref(64 + rl + 64 + 16, 0);
  for (uint32_t i = 0; i < rl; ++i) ref[64 + i] = (uint8_t)BASES[rng.next(4)];
  std::vector<uint8_t> text(ref.begin() + 64 + pos, ref.begin() + 64 + pos + L + 1);  // (one base more than the read: the deletion's)
  int nerr = 2;
  text[7] = other_base(text[7], 0); text[L - 9] = other_base(text[L - 9], 1);
  uint32_t ref_span = L;
  if (kind == 1) { text.erase(text.begin() + 20); nerr = 3; ref_span = L + 1; }  // the read skips a reference base
  text.resize(L);
  if (kind == 2) text[30] = 'N';  // (a third mismatch)
  if (kind == 3) text[30] |= 0x20;
  if (kind == 2) nerr = 3;  // (kind 3: the aligner's distance stays 2 -- it ignores case -- while the raw count is 3: the traceback runs)
  std::vector<uint8_t> raw(L + 32, 0);
  for (uint32_t i = 0; i < L; ++i) {
    const uint8_t c = text[strand ? L - 1 - i : i];
    raw[i] = !strand ? c : c == 'N' ? 'N' : (c & 0x20) ? (uint8_t)(comp(c & 0xDFu) | 0x20) : comp(c);
  }
  const std::vector<CmPlRec> pl = pack_ref(ref);
  CmDev d;
  memset(&d, 0, sizeof d);
  const uint64_t ref_off[1] = {64};
  const uint32_t ref_len[1] = {rl};
  uint32_t ro[2] = {0, L}, rlen[2] = {L, 0};
  uint8_t plain[2] = {0, 0};
  d.ref = ref.data(); d.ref_off = ref_off; d.ref_len = ref_len; d.n_seq = 1;
  d.ref_pl = pl.data() + CM_PL_LEAD; d.ref_pl_words = pl.size() - CM_PL_LEAD;
  d.rb0 = raw.data(); d.rb1 = raw.data(); d.ro0 = ro; d.ro1 = ro; d.rlen = rlen; d.n_pairs = 1;
  d.p.e = (int32_t)e;
  d.read_pl_w = (L + 31) / 32;
  std::vector<uint32_t> planes(2 * cm_read_pl_stride(d.read_pl_w) + 4, 0x5A5A5A5Au);
  d.read_pl = planes.data();
  d.read_plain = plain;
  if (L <= 64) plain[0] = (uint8_t)pack_read(d, 0, raw.data(), L, L);  // (longer reads never reach the planes instance: flag 0)
  if (kind >= 2 && kind <= 4) planes.assign(planes.size(), 0x5A5A5A5Au);
  const uint64_t dpos = (uint64_t)(pos + ref_span - 1);  // rid 0, the mapping's last reference base
  for (int on = 1; on >= 0; --on) {
    d.read_plain = on ? plain : nullptr;  // (what cmgpu_set_option "s6_planes" 0 binds)
    const CmSpan s = cm_ref_start_end(d, 0, dpos, nerr, strand, raw.data(), (int)L);
    uint32_t *o = out + (on ? 0 : 3);
    o[0] = s.rid; o[1] = s.ref_start; o[2] = s.ref_end;
  }
  out[6] = plain[0];
  out[7] = (uint32_t)nerr;
  out[8] = pos;
  return 0;
}

// Every case of tests/test_s6_planes_cpu.py in one call (what the stand-alone program runs): the number of cases, or -1 with
// bad[0..5] = L, sh, strand, mis, ref_kind, extra of the first count case that differs, or -2 with bad[0..1] = kind, strand of a
// dispatch case whose two calls differ.
extern "C" long hostemu_s6p_sweep(uint64_t seed, int32_t *bad) {
  static const uint32_t Ls[] = {17, 31, 32, 33, 50, 63, 64}, shs[] = {0, 1, 17, 31};
  long cases = 0;
  for (uint32_t L : Ls)
    for (uint32_t sh : shs)
      for (int strand = 0; strand < 2; ++strand)
        for (int mis = 0; mis <= 4; ++mis)
          for (int rk = 0; rk <= 4; ++rk)
            for (uint32_t extra = 0; extra <= 5 && L + extra <= 64; extra += 5) {
              int32_t o[5] = {-1, -1, -1, -1, -1};
              const int rc = hostemu_s6p_case(L, sh, strand, mis, rk, extra, seed, o);
              if (rc || o[0] != o[1] || o[0] != o[2] || o[0] != o[3] || o[4] != 1) {
                bad[0] = (int32_t)L; bad[1] = (int32_t)sh; bad[2] = strand; bad[3] = mis; bad[4] = rk; bad[5] = (int32_t)extra;
                return -1;
              }
              ++cases;
            }
  for (int kind = 0; kind <= 6; ++kind)
    for (int strand = 0; strand < 2; ++strand) {
      uint32_t o[9] = {0};
      const int rc = hostemu_s6p_dispatch(kind, strand, seed, o);
      const bool flag_ok = o[6] == ((kind >= 2 && kind <= 4) ? 0u : 1u);
      if (rc || o[0] != o[3] || o[1] != o[4] || o[2] != o[5] || !flag_ok) { bad[0] = kind; bad[1] = strand; return -2; }
      ++cases;
    }
  return cases;
}
