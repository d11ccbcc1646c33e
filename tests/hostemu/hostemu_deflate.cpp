// hostemu_deflate.cpp -- TEST INFRASTRUCTURE.  The device's BGZF compressor (chromap_amd/csrc/cm_deflate.h) on the host: a text cut
// into slices of CM_DF_SLICE bytes, one cm_deflate_block per slice, the blocks back to back.  The group is either emu_group.h's (64
// lanes as fibers, in ascending or descending order: a missing barrier shows as stale data under one of them) or a single lane, for
// which every barrier is empty -- the blocks must be the same bytes whatever runs them.  Every block is written into a slot with guard
// bytes around it, and so are the tokens.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../chromap_amd/csrc/cm_deflate.h"
#include "emu_group.h"

struct OneLane {
  static constexpr int G = 1;
  static constexpr int W = 1;
  uint32_t t = 0;
  void sync() {}
  void wsync() {}
  uint32_t scan(uint32_t v, uint32_t *total) { *total = v; return 0; }
  uint32_t sum(uint32_t v) { return v; }
};

// mode 0: one lane; 1 / 2: 64 lanes, ascending / descending; 3: 256 lanes (the device's group), ascending.
// Returns the number of bytes written to out, -1: out too small, -2: a block or its tokens went outside their room, -3: a block of
// CM_DF_SLOT bytes or more.  n_blocks (optional): the number of blocks.
extern "C" long hostemu_deflate(const uint8_t *text, uint64_t n, uint8_t *out, uint64_t cap, int mode, uint64_t *n_blocks) {
  static CmCrcX2n x2n;
  static bool have = false;
  if (!have) { cm_crc_x2n_table(x2n); have = true; }
  const size_t guard = 256;
  std::vector<uint8_t> slot(CM_DF_SLOT + 2 * guard);
  std::vector<uint32_t> tok(CM_DF_SLICE + 2 * 16);
  std::vector<CmDfShared> shv(1);
  CmDfShared &sh = shv[0];
  // (the slices at the alignment the device sees: the text's start is 16-byte aligned there, and so is every slice)
  std::vector<CmDf16> stage((CM_DF_SLICE + 15) / 16 + 1);
  uint64_t at = 0, nb = 0;
  for (uint64_t off = 0; off < n; off += CM_DF_SLICE, ++nb) {
    const uint32_t m = n - off < CM_DF_SLICE ? (uint32_t)(n - off) : CM_DF_SLICE;
    // an odd block's text one byte off a 16-byte boundary: the byte-wise path of the staging loop
    uint8_t *src = reinterpret_cast<uint8_t *>(stage.data()) + (nb & 1 ? 1 : 0);
    memcpy(src, text + off, m);
    memset(slot.data(), 0xA5, slot.size());
    for (uint32_t &w : tok) w = 0xA5A5A5A5u;
    memset(&sh, 0xC3, sizeof sh);  // (shared memory holds anything when a group starts)
    uint32_t total = 0;
    uint8_t *o = slot.data() + guard;
    uint32_t *tk = tok.data() + 16;
    if (mode == 0) {
      OneLane g;
      total = cm_deflate_block(g, src, m, o, tk, sh, x2n.v);
    } else if (mode == 3) {
      emu_run_group<256>([&](EmuGroup<256> &g) {
        const uint32_t r = cm_deflate_block(g, src, m, o, tk, sh, x2n.v);
        if (g.t == 255) total = r;
      });
    } else {
      emu_run_group<64>([&](EmuGroup<64> &g) {
        const uint32_t r = cm_deflate_block(g, src, m, o, tk, sh, x2n.v);
        if (g.t == 63) total = r;
      }, mode == 2);
    }
    if (total >= CM_DF_SLOT) return -3;
    for (size_t i = 0; i < guard; ++i)
      if (slot[i] != 0xA5 || slot[guard + CM_DF_SLOT + i] != 0xA5) return -2;
    for (size_t i = total; i < CM_DF_SLOT; ++i)
      if (o[i] != 0xA5) return -2;  // (nothing behind the block's own bytes either)
    for (size_t i = 0; i < 16; ++i)
      if (tok[i] != 0xA5A5A5A5u || tok[16 + CM_DF_SLICE + i] != 0xA5A5A5A5u) return -2;
    for (size_t i = m; i < CM_DF_SLICE; ++i)
      if (tk[i] != 0xA5A5A5A5u) return -2;  // (a slice of m bytes has at most m tokens)
    if (cap - at < total) return -1;
    memcpy(out + at, o, total);
    at += total;
  }
  if (n_blocks) *n_blocks = nb;
  return (long)at;
}

extern "C" uint32_t hostemu_deflate_shared_bytes() { return (uint32_t)sizeof(CmDfShared); }

// cm_df_huff alone: code lengths (<= maxbits, at most 15) of the n <= 288 symbols counted in cnt.  mode as above (0: one lane, 1 / 2: 64 lanes)
extern "C" void hostemu_df_huff(const uint32_t *cnt, uint32_t n, uint32_t maxbits, uint8_t *len, int mode) {
  std::vector<uint32_t> area(CM_DF_AREA, 0xC3C3C3C3u), blc(16, 0xC3C3C3C3u), c(cnt, cnt + n);
  if (mode == 0) {
    OneLane g;
    cm_df_huff(g, c.data(), n, maxbits, len, area.data(), blc.data());
  } else {
    emu_run_group<64>([&](EmuGroup<64> &g) { cm_df_huff(g, c.data(), n, maxbits, len, area.data(), blc.data()); }, mode == 2);
  }
}
