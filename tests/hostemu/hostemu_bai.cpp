// hostemu_bai.cpp -- TEST INFRASTRUCTURE.  The device's BAM indexer (chromap_amd/csrc/cm_bai.h, cm_tabix.hip) on the host: the same
// per-record and per-chunk functions and the same serialiser, run by plain loops in place of the kernels, std::stable_sort in place
// of the radix sort and sequential scans.  The records are taken one by one, or in waves of 64 lanes that settle their reference's
// windows and counts as the device's kernel does (one update for the wave where all its lanes have one reference, else one per
// lane), the waves and their lanes in ascending or descending order, or in blocks of 256 -- what they leave must not depend on who
// comes first.  The bytes lie in a buffer of exactly their size (one byte off an 8-byte boundary under the descending order), so
// that a sanitizer build sees every load past them.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../chromap_amd/csrc/cm_bai.h"

namespace {
struct HostAtomics {
  static void min64(unsigned long long *p, unsigned long long v) { if (v < *p) *p = v; }
};
// f(i) for i in [0, n): mode 0 ascending; 1: waves of 64 ascending; 2: everything descending; 3: blocks of 256, the last block first
template <class F>
void each(uint64_t n, int mode, F f) {
  if (mode == 2) { for (uint64_t i = n; i-- > 0;) f(i); return; }
  if (mode == 3) {
    for (uint64_t b = (n + 255) / 256; b-- > 0;)
      for (uint64_t i = b * 256; i < n && i < (b + 1) * 256; ++i) f(i);
    return;
  }
  for (uint64_t i = 0; i < n; ++i) f(i);
}
void inclusive_scan(uint32_t *v, uint64_t n) {
  for (uint64_t i = 1; i < n; ++i) v[i] += v[i - 1];
}
// k_bai_flags: the waves of 64 lanes over the records
void flags(const CmBaiArrays &d, int mode) {
  const uint64_t n_waves = (d.n_rec + 63) / 64;
  each(n_waves, mode, [&](uint64_t wv) {
    uint32_t t[64], want[64], unm[64];
    for (int l = 0; l < 64; ++l) { t[l] = ~0u; want[l] = 0; unm[l] = 0; }
    each(64, mode == 2 ? 2 : 0, [&](uint64_t l) {
      const uint64_t i = wv * 64 + l;
      if (i < d.n_rec) want[l] = cm_bai_rec_flags_core(d, i, &t[l], &unm[l]);
    });
    bool all = true;
    for (int l = 1; l < 64; ++l) all = all && t[l] == t[0];
    if (mode == 0) all = false;  // one lane: every record for itself
    if (all) {
      if (t[0] == ~0u) return;
      uint32_t mx = 0, n_unm = 0;
      for (int l = 0; l < 64; ++l) { mx = want[l] > mx ? want[l] : mx; n_unm += unm[l]; }
      CmBaiRef &r = d.ref[t[0]];
      if (mx > r.n_intv) r.n_intv = mx;
      r.n_mapped += 64u - n_unm;
      r.n_unmapped += n_unm;
      return;
    }
    each(64, mode == 2 ? 2 : 0, [&](uint64_t l) {
      if (t[l] == ~0u) return;
      CmBaiRef &r = d.ref[t[l]];
      if (want[l] > r.n_intv) r.n_intv = want[l];
      ++(unm[l] ? r.n_unmapped : r.n_mapped);
    });
  });
}
}  // namespace

// The index of the n bytes of records, record i at starts[i] (n_rec + 1 entries), whose slices of 0xff00 bytes became blocks of the
// given sizes, the first of them at file offset base.  Returns the payload's bytes in out; -1: out too small; -2: the records cannot
// be indexed, *err_word says why (record << 3 | cause); -4: something was written outside its array
extern "C" long hostemu_bai(const uint8_t *bytes_in, uint64_t n, const uint64_t *starts_in, uint64_t n_rec, uint32_t n_ref, const uint32_t *sizes, uint64_t n_blocks,
                            uint64_t base, uint8_t *out, uint64_t cap, int mode, uint64_t *err_word) {
  std::vector<uint8_t> payload;
  *err_word = CM_TBX_NO_ERROR;
  auto finish = [&]() -> long {
    if (payload.size() > cap) return -1;
    memcpy(out, payload.data(), payload.size());
    return (long)payload.size();
  };
  std::vector<CmBaiRef> ref(n_ref);
  if (n_ref) memset(ref.data(), 0, n_ref * sizeof(CmBaiRef));
  std::vector<uint64_t> lin_off((size_t)n_ref + 1, 0), lin64(1);
  if (n_rec == 0) {
    cm_bai_serialize(ref.data(), n_ref, nullptr, 0, lin64.data(), lin_off.data(), payload);
    return finish();
  }
  // (malloc, not a vector: the records' n bytes end where the allocation ends)
  const size_t shift = mode == 2 ? 1 : 0;
  uint8_t *room = static_cast<uint8_t *>(malloc(n + shift));
  if (!room) return -5;
  struct Free { uint8_t *p; ~Free() { free(p); } } free_room{room};
  uint8_t *bytes = room + shift;
  memcpy(bytes, bytes_in, n);
  std::vector<uint64_t> starts(starts_in, starts_in + n_rec + 1);
  std::vector<uint64_t> coff(n_blocks + 1, 0);
  for (uint64_t k = 0; k < n_blocks; ++k) coff[k + 1] = coff[k] + sizes[k];
  const uint32_t GUARD = 0xA5A5A5A5u;
  const size_t guard = 8;
  std::vector<uint32_t> beg_room(n_rec + 2 * guard, GUARD), end_room(n_rec + 2 * guard, GUARD), tid_room(n_rec + 2 * guard, GUARD), cidx_room(n_rec + 2 * guard, GUARD);
  auto guards_ok = [&](const std::vector<uint32_t> &v) {
    for (size_t i = 0; i < guard; ++i)
      if (v[i] != GUARD || v[guard + n_rec + i] != GUARD) return false;
    return true;
  };
  unsigned long long err = CM_TBX_NO_ERROR;
  CmBaiArrays d = {};
  d.t.p = bytes;
  d.t.n = n;
  d.t.n_blocks = n_blocks;
  d.t.coff = coff.data();
  d.t.base = base;
  d.n_rec = n_rec;
  d.starts = starts.data();
  d.n_ref = n_ref;
  d.beg = beg_room.data() + guard;
  d.end = end_room.data() + guard;
  d.tid = tid_room.data() + guard;
  d.cidx = cidx_room.data() + guard;
  d.err = &err;
  d.ref = ref.data();
  // 1. per record
  each(n_rec, mode, [&](uint64_t i) { cm_bai_rec_parse<HostAtomics>(d, i); });
  if (err != CM_TBX_NO_ERROR) { *err_word = err; return -2; }
  // 2. references, raw chunks
  flags(d, mode);
  inclusive_scan(d.cidx, n_rec);
  const uint32_t n_raw = d.cidx[n_rec - 1];
  for (uint32_t r = 0; r < n_ref; ++r) lin_off[r + 1] = lin_off[r] + ref[r].n_intv;
  const uint64_t n_win = lin_off[n_ref];
  std::vector<unsigned long long> lin(n_win + 2, ~0ull);
  std::vector<uint64_t> ckey(n_raw), cbeg(n_raw), cend(n_raw), skey(n_raw);
  std::vector<uint32_t> cval(n_raw), perm(n_raw), mflag(n_raw);
  d.lin_off = lin_off.data();
  d.lin = lin.data();
  d.ckey = ckey.data();
  d.cbeg = cbeg.data();
  d.cend = cend.data();
  d.cval = cval.data();
  each(n_rec, mode, [&](uint64_t i) { cm_bai_rec_emit<HostAtomics>(d, i); });
  if (lin[n_win] != ~0ull || lin[n_win + 1] != ~0ull) return -4;
  if (!guards_ok(beg_room) || !guards_ok(end_room) || !guards_ok(tid_room) || !guards_ok(cidx_room)) return -4;
  for (uint64_t w = n_win; w-- > 1;)  // (the device's back-fill: one reverse minimum scan over all references' windows)
    if (lin[w] < lin[w - 1]) lin[w - 1] = lin[w];
  // 3. raw chunks
  perm = cval;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return ckey[a] < ckey[b]; });
  for (uint32_t j = 0; j < n_raw; ++j) skey[j] = ckey[perm[j]];
  each(n_raw, mode, [&](uint64_t j) { mflag[j] = cm_tbx_chunk_flag(skey.data(), perm.data(), cbeg.data(), cend.data(), j); });
  inclusive_scan(mflag.data(), n_raw);
  const uint32_t n_merged = mflag[n_raw - 1];
  std::vector<CmTbxChunk> ch(n_merged);
  each(n_raw, mode, [&](uint64_t j) { cm_tbx_chunk_emit(skey.data(), perm.data(), cbeg.data(), cend.data(), mflag.data(), n_raw, j, ch.data()); });
  // 4. the payload
  lin64.assign(lin.begin(), lin.begin() + n_win);
  lin64.push_back(0);
  cm_bai_serialize(ref.data(), n_ref, ch.data(), n_merged, lin64.data(), lin_off.data(), payload);
  return finish();
}
