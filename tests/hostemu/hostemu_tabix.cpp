// hostemu_tabix.cpp -- TEST INFRASTRUCTURE.  The device's tabix indexer (chromap_amd/csrc/cm_tabix.h, cm_tabix.hip) on the host: the
// same tile, line and chunk functions and the same serialiser, run by plain loops in place of the kernels, std::stable_sort in place of
// the radix sort and sequential scans.  The tiles' group is one lane, or emu_group.h's 64 lanes in ascending or descending order, or
// 256 lanes (the device's group); the per-line and per-chunk loops run forwards, or backwards under the descending order -- what
// they leave must not depend on who comes first.  The line-start array has guard words around it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../chromap_amd/csrc/cm_tabix.h"
#include "emu_group.h"

struct OneLane {
  static constexpr int G = 1;
  uint32_t t = 0;
  uint32_t scan(uint32_t v, uint32_t *total) { *total = v; return 0; }
  uint32_t sum(uint32_t v) { return v; }
};
struct HostAtomics {
  static void min64(unsigned long long *p, unsigned long long v) { if (v < *p) *p = v; }
};

template <class F>
static void each(uint64_t n, bool backwards, F f) {
  if (backwards) for (uint64_t i = n; i-- > 0;) f(i);
  else for (uint64_t i = 0; i < n; ++i) f(i);
}
static void inclusive_scan(uint32_t *v, uint64_t n) {
  for (uint64_t i = 1; i < n; ++i) v[i] += v[i - 1];
}

// mode 0: one lane; 1 / 2: 64 lanes, ascending / descending (2: the item loops backwards too, and the text one byte off an 8-byte
// boundary: the byte-wise path of the newline search); 3: 256 lanes.
// Returns the payload's bytes in out; -1: out too small; -2: the text cannot be indexed, *err_word says why (line << 3 | cause);
// -3: no final newline; -4: something was written outside its array
extern "C" long hostemu_tabix(const uint8_t *text_in, uint64_t n, const uint32_t *sizes, uint64_t n_blocks, uint64_t base, uint8_t *out, uint64_t cap,
                              int mode, uint64_t *err_word) {
  std::vector<uint8_t> payload;
  *err_word = CM_TBX_NO_ERROR;
  const bool back = mode == 2;
  auto finish = [&]() -> long {
    if (payload.size() > cap) return -1;
    memcpy(out, payload.data(), payload.size());
    return (long)payload.size();
  };
  if (n == 0) {
    cm_tbx_serialize(nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, payload);
    return finish();
  }
  std::vector<uint64_t> room(n / 8 + 4);
  uint8_t *text = reinterpret_cast<uint8_t *>(room.data()) + (back ? 1 : 0);
  memcpy(text, text_in, n);
  std::vector<uint64_t> coff(n_blocks + 1, 0);
  for (uint64_t k = 0; k < n_blocks; ++k) coff[k + 1] = coff[k] + sizes[k];
  CmTbxArrays d = {};
  d.t.p = text;
  d.t.n = n;
  d.t.n_blocks = n_blocks;
  d.t.coff = coff.data();
  d.t.base = base;
  // 1. line starts
  const uint64_t n_tiles = (n + CM_TBX_TILE - 1) / CM_TBX_TILE;
  std::vector<uint64_t> tcnt(n_tiles + 1, 0), toff(n_tiles + 1, 0);
  auto tiles = [&](auto body) {
    each(n_tiles, back, [&](uint64_t tile) {
      if (mode == 0) { OneLane g; body(g, tile); }
      else if (mode == 3) emu_run_group<256>([&](EmuGroup<256> &g) { body(g, tile); });
      else emu_run_group<64>([&](EmuGroup<64> &g) { body(g, tile); }, back);
    });
  };
  tiles([&](auto &g, uint64_t tile) {
    const uint32_t c = cm_tbx_tile_count(g, text, n, tile);
    if (g.t == 0) tcnt[tile] = c;
  });
  for (uint64_t t = 0; t < n_tiles; ++t) toff[t + 1] = toff[t] + tcnt[t];
  const uint64_t n_lines = toff[n_tiles];
  if (text[n - 1] != '\n') return -3;
  const size_t guard = 8;
  const uint64_t GUARD = 0xA5A5A5A5A5A5A5A5ull;
  std::vector<uint64_t> lstart_room(n_lines + 1 + 2 * guard, GUARD);
  uint64_t *lstart = lstart_room.data() + guard;
  lstart[0] = 0;
  tiles([&](auto &g, uint64_t tile) { cm_tbx_tile_starts(g, text, n, tile, toff[tile], lstart); });
  for (size_t i = 0; i < guard; ++i)
    if (lstart_room[i] != GUARD || lstart_room[guard + n_lines + 1 + i] != GUARD) return -4;
  if (lstart[n_lines] != n) return -4;
  // 2. per line
  std::vector<uint32_t> beg(n_lines), end(n_lines), tid(n_lines), cidx(n_lines);
  unsigned long long err = CM_TBX_NO_ERROR;
  d.n_lines = n_lines;
  d.lstart = lstart;
  d.beg = beg.data();
  d.end = end.data();
  d.tid = tid.data();
  d.cidx = cidx.data();
  d.err = &err;
  each(n_lines, back, [&](uint64_t i) { cm_tbx_line_parse<HostAtomics>(d, i); });
  inclusive_scan(tid.data(), n_lines);
  if (err != CM_TBX_NO_ERROR) { *err_word = err; return -2; }
  const uint32_t n_ref = tid[n_lines - 1];
  std::vector<CmTbxRef> ref(n_ref);
  memset(ref.data(), 0, n_ref * sizeof(CmTbxRef));
  d.ref = ref.data();
  each(n_lines, back, [&](uint64_t i) {
    uint32_t t;
    unsigned long long e = CM_TBX_NO_ERROR;
    const uint32_t want = cm_tbx_line_flags_core(d, i, &t, &e);
    HostAtomics::min64(&err, e);
    if (want > ref[t].n_intv) ref[t].n_intv = want;
  });
  inclusive_scan(cidx.data(), n_lines);
  if (err != CM_TBX_NO_ERROR) { *err_word = err; return -2; }
  const uint32_t n_raw = cidx[n_lines - 1];
  std::vector<uint64_t> name_off(n_ref + 1, 0), lin_off(n_ref + 1, 0);
  for (uint32_t r = 0; r < n_ref; ++r) {
    name_off[r + 1] = name_off[r] + ref[r].name_len;
    lin_off[r + 1] = lin_off[r] + ref[r].n_intv;
  }
  std::vector<uint8_t> names(name_off[n_ref] + 1);
  for (uint32_t r = 0; r < n_ref; ++r) memcpy(names.data() + name_off[r], text + ref[r].name_at, ref[r].name_len);
  for (uint32_t r = 0; r < n_ref; ++r)  // (a plain search: the test texts have few names)
    for (uint32_t q = 0; q < r; ++q)
      if (ref[q].name_len == ref[r].name_len && !memcmp(names.data() + name_off[q], names.data() + name_off[r], ref[r].name_len)) {
        *err_word = (uint64_t)ref[r].first_line << 3 | CM_TBX_E_RECUR;
        return -2;
      }
  std::vector<unsigned long long> lin(lin_off[n_ref] + 1, ~0ull);
  std::vector<uint64_t> ckey(n_raw), cbeg(n_raw), cend(n_raw), skey(n_raw);
  std::vector<uint32_t> cval(n_raw), perm(n_raw), mflag(n_raw);
  d.lin_off = lin_off.data();
  d.lin = lin.data();
  d.ckey = ckey.data();
  d.cbeg = cbeg.data();
  d.cend = cend.data();
  d.cval = cval.data();
  each(n_lines, back, [&](uint64_t i) { cm_tbx_line_emit<HostAtomics>(d, i); });
  for (uint64_t w = lin_off[n_ref]; w-- > 1;)
    if (lin[w] < lin[w - 1]) lin[w - 1] = lin[w];
  // 3. raw chunks
  perm = cval;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return ckey[a] < ckey[b]; });
  for (uint32_t j = 0; j < n_raw; ++j) skey[j] = ckey[perm[j]];
  each(n_raw, back, [&](uint64_t j) { mflag[j] = cm_tbx_chunk_flag(skey.data(), perm.data(), cbeg.data(), cend.data(), j); });
  inclusive_scan(mflag.data(), n_raw);
  const uint32_t n_merged = mflag[n_raw - 1];
  std::vector<CmTbxChunk> ch(n_merged);
  each(n_raw, back, [&](uint64_t j) { cm_tbx_chunk_emit(skey.data(), perm.data(), cbeg.data(), cend.data(), mflag.data(), n_raw, j, ch.data()); });
  // 4. the payload
  std::vector<uint64_t> lin64(lin.begin(), lin.end());
  cm_tbx_serialize(ref.data(), n_ref, n_lines, names.data(), name_off.data(), ch.data(), n_merged, lin64.data(), lin_off.data(), payload);
  return finish();
}

extern "C" uint32_t hostemu_tabix_reg2bin(uint32_t beg, uint32_t end) { return cm_tbx_reg2bin(beg, end); }
