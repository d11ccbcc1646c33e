// cm_deflate.h -- the text store compressed into BGZF blocks (SAM spec 4.1) on the device: the counterpart of cm_inflate.h.  Block i
// holds the text bytes [i * 0xff00, (i + 1) * 0xff00): an 18-byte header with the 'BC' field, one raw DEFLATE stream (RFC 1951), the
// CRC-32 and the size of the text.  ONE WORKGROUP per block (a group of cm_coop.h's kind: t, sync(), wsync(), scan(), sum()) with the
// slice in shared memory:
//
//  1. CRC-32 of the slice (cm_bgzf_crc of cm_inflate.h).
//  2. LZ77, a tile of CM_DF_T positions at a time.  A table of 2^CM_DF_HBITS entries in shared memory, indexed by a hash of the 4 bytes at
//     a position, holds the LAST position that was entered (an atomic maximum: the result does not depend on who comes first).  The
//     positions of a tile look the table up and enter themselves 32 at a time, so a position finds the most recent earlier position
//     with its hash that lies before its own group of 32 -- the same 4 bytes one line up are 40 to 300 bytes back.  What a group of 32
//     cannot see in itself is mostly runs of one byte: the candidate at distance 1 is checked beside the table's.  The longer of the
//     two matches counts, at least CM_DF_MIN bytes long, at most 258, at most 32768 back.
//  3. The greedy parse next(p) = p + (length of p's match, or 1): the chain from the tile's entry position is marked by pointer jumping
//     inside the tile (8 doublings for 256 positions), the marked positions become tokens in global scratch and are counted per symbol.
//  4. One dynamic-Huffman block: code lengths from the counts by Huffman's algorithm over the sorted symbols (one lane; two queues),
//     limited to 15 bits (7 for the code-length code) by zlib's rule for an over-long tree; a code with a single symbol gets a second one
//     so that every code is complete.  The header sends the lengths one by one (no symbols 16-18).  The code words' places are a prefix
//     sum of their lengths, every lane ORs its words into place -- in the slice's own shared memory, which is free by then: a block
//     that would not come out smaller than the slice is written as one stored block instead, so the coded bytes always fit there.
//
// Nothing depends on the number of lanes or on their timing: the blocks are a function of the text alone, and the same text compiles
// for the host (tests/hostemu/hostemu_deflate.cpp: against zlib and against cm_inflate.h).
// Every loop is bounded by the slice size; a block is written inside out[0 .. CM_DF_SLOT) only.
#ifndef CM_DEFLATE_H_
#define CM_DEFLATE_H_

#include <stdint.h>

#include "cm_inflate.h"
#include "cm_types.h"

#define CM_DF_SLICE 0xff00u   // text bytes per block (bgzip's)
#define CM_DF_SLOT 65536u     // a block is smaller than this (a stored slice: 0xff00 + 5 + 26)
#define CM_DF_T 256u          // positions per tile
#define CM_DF_SUB 32u         // positions that look up and enter the hash table together
#define CM_DF_HBITS 11
#define CM_DF_MIN 4u
#define CM_DF_MAXLEN 258u
#define CM_DF_MAXDIST 32768u
#define CM_DF_PAD 32u         // zero bytes behind the slice in shared memory
#define CM_DF_AREA 2048u      // words of the work area (the hash table; the CRC's tables; the Huffman builder's)
#define CM_DF_TOK_LIT 0x80000000u  // token: a literal (bits 0..7), or a match: length in bits 16..24, distance - 1 in bits 0..15

#ifdef __HIP_DEVICE_COMPILE__
#define CM_DF_AMAX(p, v) atomicMax((p), (v))
#define CM_DF_AADD(p, v) atomicAdd((p), (v))
#define CM_DF_AOR(p, v) atomicOr((p), (v))
#else  // (the host's lanes take turns)
#define CM_DF_AMAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define CM_DF_AADD(p, v) (*(p) += (v))
#define CM_DF_AOR(p, v) (*(p) |= (v))
#endif

// the workgroup's shared memory (78 KiB: two workgroups per compute unit)
struct alignas(16) CmDfShared {
  uint32_t win32[(CM_DF_SLICE + CM_DF_PAD) / 4u];  // the slice and CM_DF_PAD zero bytes; later the coded bytes
  uint32_t area[CM_DF_AREA];
  uint32_t ll_cnt[288], d_cnt[32], cl_cnt[20];
  uint16_t ll_code[288], d_code[32], cl_code[20];
  uint8_t ll_len[288], d_len[32], cl_len[20];
  uint16_t mlen[CM_DF_T], mdist[CM_DF_T], jmp[2][CM_DF_T];
  uint8_t mark[CM_DF_T];
  uint32_t blc[16];
  uint32_t carry;
};

struct alignas(16) CmDf16 { uint32_t x, y, z, w; };
CM_HD uint64_t cm_df_ld8(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
CM_HD uint32_t cm_df_ld4(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
CM_HD uint32_t cm_df_log2(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }  // x > 0

// bytes that win[q ..] and win[p ..] share, at most maxl (q < p; 32 at a time: behind the slice lie CM_DF_PAD zero bytes, and a count
// beyond maxl is cut)
CM_HD uint32_t cm_df_match(const uint8_t *win, uint32_t q, uint32_t p, uint32_t maxl) {
  uint32_t l = 0;
  while (l < maxl) {  // (the four loads of a side are asked for together: a step waits for shared memory once)
    uint64_t x[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) x[k] = cm_df_ld8(win + q + l + 8u * k) ^ cm_df_ld8(win + p + l + 8u * k);
    if (x[0] | x[1] | x[2] | x[3]) {
      l += x[0] ? (uint32_t)__builtin_ctzll(x[0]) >> 3 : x[1] ? 8u + ((uint32_t)__builtin_ctzll(x[1]) >> 3)
           : x[2] ? 16u + ((uint32_t)__builtin_ctzll(x[2]) >> 3) : 24u + ((uint32_t)__builtin_ctzll(x[3]) >> 3);
      break;
    }
    l += 32;
  }
  return l < maxl ? l : maxl;
}

// symbol and extra bits of a match length (3..258) and of a distance (1..32768): RFC 1951 3.2.5 in closed form, the inverse of
// cm_inf_symbols'
CM_HD uint32_t cm_df_len_sym(uint32_t len, uint32_t *nx, uint32_t *xv) {
  const uint32_t x = len - 3u;
  if (x < 8u || len == 258u) { *nx = 0; *xv = 0; return len == 258u ? 285u : 257u + x; }
  const uint32_t e = cm_df_log2(x) - 2u;
  *nx = e;
  *xv = x & ((1u << e) - 1u);
  return 257u + 4u * e + (x >> e);  // (x >> e is 4..7)
}
CM_HD uint32_t cm_df_dist_sym(uint32_t dist, uint32_t *nx, uint32_t *xv) {
  const uint32_t d = dist - 1u;
  if (d < 4u) { *nx = 0; *xv = 0; return d; }
  const uint32_t e = cm_df_log2(d) - 1u;
  *nx = e;
  *xv = d & ((1u << e) - 1u);
  return 2u * e + 2u + ((d >> e) & 1u);
}
CM_HD uint32_t cm_df_len_extra(uint32_t sym) {  // extra bits of literal / length symbol sym
  if (sym < 265u || sym >= 285u) return 0;
  return (sym - 261u) >> 2;
}
CM_HD uint32_t cm_df_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }

// nbits (<= 48) bits of val at bit `at` of w (zero there before)
CM_HD void cm_df_put(uint32_t *w, uint32_t at, uint64_t val, uint32_t nbits) {
  if (!nbits) return;
  const uint32_t wi = at >> 5, sh = at & 31u;
  const uint64_t lo = val << sh;
  const uint32_t hi = sh ? (uint32_t)(val >> (64u - sh)) : 0u;
  if ((uint32_t)lo) CM_DF_AOR(&w[wi], (uint32_t)lo);
  if (lo >> 32) CM_DF_AOR(&w[wi + 1u], (uint32_t)(lo >> 32));
  if (hi) CM_DF_AOR(&w[wi + 2u], hi);
}

// Code lengths (<= maxbits) of the n symbols counted in cnt; an unused symbol gets 0.  area: 1008 words, blc: 16 words.
template <class GT>
CM_HD void cm_df_huff(GT &g, const uint32_t *cnt, uint32_t n, uint32_t maxbits, uint8_t *len, uint32_t *area, uint32_t *blc) {
  const uint32_t G = (uint32_t)GT::G;
  uint32_t *wt = area;                                             // 576: weights, later depths, of leaves and inner nodes
  uint16_t *order = reinterpret_cast<uint16_t *>(area + 576);      // 288: the used symbols by (count, symbol)
  uint16_t *par = reinterpret_cast<uint16_t *>(area + 720);        // 576
  uint32_t mine = 0;
  for (uint32_t i = g.t; i < n; i += G) {
    len[i] = 0;
    const uint32_t ci = cnt[i];
    if (!ci) continue;
    uint32_t r = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < n; ++j) {
      const uint32_t cj = cnt[j];
      r += cj && (cj < ci || (cj == ci && j < i)) ? 1u : 0u;
    }
    order[r] = (uint16_t)i;
    ++mine;
  }
  const uint32_t nu = g.sum(mine);
  g.sync();
  if (g.t == 0 && nu == 1) {  // a second symbol: every code is complete
    const uint32_t s = order[0];
    len[s] = 1;
    len[s ? 0u : 1u] = 1;
  }
  if (g.t == 0 && nu >= 2) {
    for (uint32_t k = 0; k < nu; ++k) wt[k] = cnt[order[k]];
    // the two lightest of: the next leaf (li), the next inner node not yet taken (ii); a leaf first where they weigh the same
    uint32_t li = 0, ii = nu;
    for (uint32_t ni = nu; ni < 2u * nu - 1u; ++ni) {
      uint32_t sum = 0;
      for (int k = 0; k < 2; ++k) {
        uint32_t a;
        if (li < nu && (ii >= ni || wt[li] <= wt[ii])) a = li++;
        else a = ii++;
        sum += wt[a];
        par[a] = (uint16_t)ni;
      }
      wt[ni] = sum;
    }
    const uint32_t root = 2u * nu - 2u;
    wt[root] = 0;
    for (uint32_t v = root; v-- > 0;) wt[v] = wt[par[v]] + 1u;  // (a parent is made after its children)
    for (uint32_t l = 0; l < 16; ++l) blc[l] = 0;
    for (uint32_t k = 0; k < nu; ++k) ++blc[wt[k] < maxbits ? wt[k] : maxbits];
    // A tree deeper than maxbits: with its deep leaves cut to maxbits the code words no longer fit -- by `over` words of maxbits bits
    // (the Kraft sum in units of 2^-maxbits).  One step of zlib's repair (gen_bitlen) takes one such unit back: a leaf of the deepest
    // level above maxbits that has one moves a level down, and one of the leaves at maxbits becomes its brother there.
    uint32_t kraft = 0;
    for (uint32_t l = 1; l <= maxbits; ++l) kraft += blc[l] << (maxbits - l);
    for (uint32_t over = kraft > (1u << maxbits) ? kraft - (1u << maxbits) : 0u; over > 0; --over) {
      uint32_t bits = maxbits - 1u;
      while (bits > 1u && blc[bits] == 0) --bits;
      --blc[bits];
      blc[bits + 1u] += 2;
      --blc[maxbits];
    }
    uint32_t k = 0;  // the longest code words to the rarest symbols
    for (uint32_t bits = maxbits; bits >= 1u; --bits)
      for (uint32_t q = 0; q < blc[bits] && k < nu; ++q) len[order[k++]] = (uint8_t)bits;
  }
  g.sync();
}

// the canonical code words of the lengths, first bit lowest (as they go into the stream)
template <class GT>
CM_HD void cm_df_codes(GT &g, const uint8_t *len, uint32_t n, uint16_t *code, uint32_t *blc) {
  const uint32_t G = (uint32_t)GT::G;
  if (g.t == 0) {
    uint32_t c[16];
    for (uint32_t l = 0; l < 16; ++l) c[l] = 0;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t li = len[i];
#pragma unroll
      for (uint32_t l = 1; l < 16; ++l) c[l] += l == li ? 1u : 0u;
    }
    uint32_t next = 0;
    blc[0] = 0;
#pragma unroll
    for (uint32_t l = 1; l < 16; ++l) {
      next = (next + c[l - 1]) << 1;
      blc[l] = next;
    }
  }
  g.sync();
  for (uint32_t i = g.t; i < n; i += G) {
    const uint32_t l = len[i];
    uint32_t c = 0;
    if (l) {
      c = blc[l];
#pragma unroll 4
      for (uint32_t j = 0; j < i; ++j) c += len[j] == l ? 1u : 0u;
      c = cm_inf_rev32(c) >> (32u - l);
    }
    code[i] = (uint16_t)c;
  }
  g.sync();
}

// the 18 bytes in front of a block's DEFLATE stream, and the 8 behind it
CM_HD void cm_df_bgzf_header(uint8_t *out, uint32_t total) {
  const uint8_t h[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
  for (int i = 0; i < 16; ++i) out[i] = h[i];
  out[16] = (uint8_t)((total - 1u) & 0xffu);
  out[17] = (uint8_t)((total - 1u) >> 8);
}
CM_HD void cm_df_bgzf_trailer(uint8_t *out, uint32_t crc, uint32_t isize) {
  for (int i = 0; i < 4; ++i) { out[i] = (uint8_t)(crc >> (8 * i)); out[4 + i] = (uint8_t)(isize >> (8 * i)); }
}

// the group's first wave part as a group of its own (the rest of the group waits at a barrier meanwhile)
template <class GT>
struct CmDfWavePart {
  static constexpr int G = GT::W;
  GT &g;
  uint32_t t;
  CM_HD explicit CmDfWavePart(GT &g_) : g(g_), t(g_.t) {}
  CM_HD void sync() { g.wsync(); }
};

// text[0 .. n) (1 <= n <= CM_DF_SLICE) -> one BGZF block at out; returns its size (< CM_DF_SLOT), the same in every lane.
// tok: n words of global scratch of this group; x2n: cm_crc_x2n_table's 32 words where every lane can read them (the device: shared memory).
template <class GT>
CM_HD uint32_t cm_deflate_block(GT &g, const uint8_t *text, uint32_t n, uint8_t *out, uint32_t *tok, CmDfShared &sh, const uint32_t *x2n) {
  const uint32_t G = (uint32_t)GT::G, W = (uint32_t)GT::W, T = CM_DF_T;
  uint8_t *win = reinterpret_cast<uint8_t *>(sh.win32);
  // ---- the slice into shared memory, zero bytes behind it
  if ((reinterpret_cast<uintptr_t>(text) & 15u) == 0) {
    const CmDf16 *src = reinterpret_cast<const CmDf16 *>(text);
    CmDf16 *dst = reinterpret_cast<CmDf16 *>(sh.win32);
    const uint32_t n16 = n / 16u;
    for (uint32_t i = g.t; i < n16; i += G) dst[i] = src[i];
    for (uint32_t i = n16 * 16u + g.t; i < n; i += G) win[i] = text[i];
  } else {
    for (uint32_t i = g.t; i < n; i += G) win[i] = text[i];
  }
  for (uint32_t i = g.t; i < CM_DF_PAD; i += G) win[n + i] = 0;
  // ---- CRC-32
  uint32_t *crc_tab = sh.area, *red = sh.area + 256;  // (red: W words)
  for (uint32_t i = g.t; i < 256u; i += G) crc_tab[i] = cm_crc32_entry(i);
  g.sync();
  if (g.t < W) {  // (cm_bgzf_crc is written for a wave: its last step reads every lane's word in one go)
    CmDfWavePart<GT> wp(g);
    const uint32_t v = cm_bgzf_crc(wp, win, n, crc_tab, x2n, red);
    if (g.t == 0) sh.carry = v;
  }
  g.sync();
  const uint32_t crc = sh.carry;
  g.sync();
  // ---- tokens
  uint32_t *tab = sh.area;
  for (uint32_t i = g.t; i < CM_DF_AREA; i += G) tab[i] = 0;
  for (uint32_t i = g.t; i < 288u; i += G) sh.ll_cnt[i] = i == 256u ? 1u : 0u;  // (the end-of-block symbol)
  for (uint32_t i = g.t; i < 32u; i += G) sh.d_cnt[i] = 0;
  if (g.t == 0) sh.carry = 0;
  g.sync();
  uint32_t entry = 0, ntok = 0;  // the chain's first position at or behind the tile's start, relative to it
  for (uint32_t base = 0; base < n; base += T) {
    const uint32_t tn = n - base < T ? n - base : T;
    // the table: CM_DF_SUB positions look up, then enter themselves -- the first wave part alone (a lane keeps its positions' hashes
    // in registers: a step is one table read and one atomic), the others wait at the barrier below
    if (g.t < W) {
      constexpr uint32_t PER = (CM_DF_SUB + (uint32_t)GT::W - 1u) / (uint32_t)GT::W;  // positions per lane and step
      constexpr uint32_t STEPS = CM_DF_T / CM_DF_SUB;
      uint16_t hreg[STEPS * PER];
#pragma unroll
      for (uint32_t s = 0; s < STEPS; ++s)
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
          const uint32_t j = g.t + k * W, p = base + s * CM_DF_SUB + j;
          hreg[s * PER + k] = j < CM_DF_SUB && p + 4u <= n ? (uint16_t)((cm_df_ld4(win + p) * 2654435761u) >> (32 - CM_DF_HBITS)) : (uint16_t)0xffffu;
        }
#pragma unroll
      for (uint32_t s = 0; s < STEPS; ++s) {
        if (s * CM_DF_SUB >= tn) break;
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
          const uint32_t j = g.t + k * W, i = s * CM_DF_SUB + j, h = hreg[s * PER + k];
          if (j < CM_DF_SUB && i < tn) sh.mdist[i] = h != 0xffffu ? (uint16_t)tab[h] : (uint16_t)0;
        }
        g.wsync();
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
          const uint32_t j = g.t + k * W, i = s * CM_DF_SUB + j, h = hreg[s * PER + k];
          if (j < CM_DF_SUB && i < tn && h != 0xffffu) CM_DF_AMAX(&tab[h], base + i + 1u);
        }
        g.wsync();
      }
    }
    g.sync();
    if (entry >= T) { entry -= T; continue; }  // (a match of 257 or 258 bytes from the tile before's last positions)
    // the matches of the positions from `entry` on
    for (uint32_t i = g.t; i < tn; i += G) {
      sh.mark[i] = i == entry ? 1 : 0;
      if (i < entry) continue;
      const uint32_t p = base + i, maxl = n - p < CM_DF_MAXLEN ? n - p : CM_DF_MAXLEN;
      const uint32_t c = sh.mdist[i];
      uint32_t best = 0, dist = 0;
      if (c && p + 1u - c <= CM_DF_MAXDIST) { best = cm_df_match(win, c - 1u, p, maxl); dist = p + 1u - c; }
      if (p > 0 && win[p - 1u] == win[p]) {
        const uint32_t l1 = cm_df_match(win, p - 1u, p, maxl);
        if (l1 >= best) { best = l1; dist = 1; }
      }
      if (best < CM_DF_MIN) best = 0;
      sh.mlen[i] = (uint16_t)best;
      sh.mdist[i] = (uint16_t)(dist - 1u);
      const uint32_t nx = i + (best ? best : 1u);
      sh.jmp[0][i] = (uint16_t)(nx < T ? nx : T);
    }
    g.sync();
    // the chain from `entry`: after round r the first 2^(r+1) of its positions are marked, jmp holds 2^(r+1) steps
    for (uint32_t r = 0; r < 8u; ++r) {
      const uint16_t *ja = sh.jmp[r & 1u];
      uint16_t *jb = sh.jmp[(r & 1u) ^ 1u];
      for (uint32_t i = g.t; i < tn; i += G) {
        if (i < entry) continue;
        const uint32_t j = ja[i];
        if (sh.mark[i] && j < tn) sh.mark[j] = 1;  // (a mark that is seen early only marks further along the same chain)
        jb[i] = j < tn ? ja[j] : (uint16_t)T;
      }
      g.sync();
    }
    // the marked positions: tokens, counts, and where the chain enters the next tile
    for (uint32_t i0 = 0; i0 < tn; i0 += G) {
      const uint32_t i = i0 + g.t;
      const bool m = i < tn && i >= entry && sh.mark[i];
      uint32_t tot;
      const uint32_t at = ntok + g.scan(m ? 1u : 0u, &tot);
      if (m) {
        const uint32_t len = sh.mlen[i];
        if (len) {
          uint32_t nx, xv;
          const uint32_t d1 = sh.mdist[i];
          tok[at] = len << 16 | d1;
          CM_DF_AADD(&sh.ll_cnt[cm_df_len_sym(len, &nx, &xv)], 1u);
          CM_DF_AADD(&sh.d_cnt[cm_df_dist_sym(d1 + 1u, &nx, &xv)], 1u);
        } else {
          const uint32_t b = win[base + i];
          tok[at] = CM_DF_TOK_LIT | b;
          CM_DF_AADD(&sh.ll_cnt[b], 1u);
        }
        CM_DF_AMAX(&sh.carry, i + (len ? len : 1u));
      }
      ntok += tot;
    }
    g.sync();
    entry = sh.carry - T;  // (carry >= tn; what it is worth behind the last tile is not used)
    g.sync();
    if (g.t == 0) sh.carry = 0;
  }
  g.sync();
  // ---- the codes
  cm_df_huff(g, sh.ll_cnt, 286u, 15u, sh.ll_len, sh.area, sh.blc);
  cm_df_huff(g, sh.d_cnt, 30u, 15u, sh.d_len, sh.area, sh.blc);
  uint32_t hlit = 257u, hdist = 1u;
#pragma unroll 4
  for (uint32_t i = 257u; i < 286u; ++i) hlit = sh.ll_len[i] ? i + 1u : hlit;
#pragma unroll 4
  for (uint32_t i = 1u; i < 30u; ++i) hdist = sh.d_len[i] ? i + 1u : hdist;
  for (uint32_t i = g.t; i < 20u; i += G) sh.cl_cnt[i] = 0;
  g.sync();
  for (uint32_t k = g.t; k < hlit + hdist; k += G) CM_DF_AADD(&sh.cl_cnt[k < hlit ? sh.ll_len[k] : sh.d_len[k - hlit]], 1u);
  g.sync();
  cm_df_huff(g, sh.cl_cnt, 19u, 7u, sh.cl_len, sh.area, sh.blc);
  cm_df_codes(g, sh.ll_len, 286u, sh.ll_code, sh.blc);
  cm_df_codes(g, sh.d_len, 30u, sh.d_code, sh.blc);
  cm_df_codes(g, sh.cl_len, 19u, sh.cl_code, sh.blc);
  // the order in which the code-length code's lengths are sent (5-bit fields, as in cm_inf_header)
  const uint64_t clord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t clord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  uint32_t hclen = 4;
  for (uint32_t i = 4; i < 19u; ++i) {
    const uint32_t which = (uint32_t)((i < 12 ? clord_lo >> (5 * i) : clord_hi >> (5 * (i - 12))) & 31ull);
    hclen = sh.cl_len[which] ? i + 1u : hclen;
  }
  // ---- the size of the coded block
  uint32_t my_bits = 0;
  for (uint32_t k = g.t; k < hlit + hdist; k += G) my_bits += sh.cl_len[k < hlit ? sh.ll_len[k] : sh.d_len[k - hlit]];
  for (uint32_t i = g.t; i < 286u; i += G) my_bits += sh.ll_cnt[i] * (sh.ll_len[i] + cm_df_len_extra(i));
  for (uint32_t i = g.t; i < 30u; i += G) my_bits += sh.d_cnt[i] * (sh.d_len[i] + cm_df_dist_extra(i));
  const uint32_t head_bits = 17u + 3u * hclen;
  const uint32_t coded = (head_bits + g.sum(my_bits) + 7u) / 8u;
  g.sync();
  uint32_t payload;
  if (coded < n) {
    payload = coded;
    uint32_t *w = sh.win32;
    for (uint32_t i = g.t; i < (coded + 3u) / 4u; i += G) w[i] = 0;
    g.sync();
    if (g.t == 0) {
      cm_df_put(w, 0, 1u | 2u << 1 | (hlit - 257u) << 3 | (hdist - 1u) << 8 | (hclen - 4u) << 13, 17u);
      for (uint32_t i = 0; i < hclen; ++i) {
        const uint32_t which = (uint32_t)((i < 12 ? clord_lo >> (5 * i) : clord_hi >> (5 * (i - 12))) & 31ull);
        cm_df_put(w, 17u + 3u * i, sh.cl_len[which], 3u);
      }
    }
    uint32_t at = head_bits;
    for (uint32_t k0 = 0; k0 < hlit + hdist; k0 += G) {
      const uint32_t k = k0 + g.t;
      const uint32_t l = k < hlit ? sh.ll_len[k] : k < hlit + hdist ? sh.d_len[k - hlit] : 0u;
      const uint32_t nb = k < hlit + hdist ? sh.cl_len[l] : 0u;
      uint32_t tot;
      const uint32_t o = g.scan(nb, &tot);
      cm_df_put(w, at + o, sh.cl_code[l], nb);
      at += tot;
    }
    for (uint32_t k0 = 0; k0 < ntok; k0 += G) {
      const uint32_t k = k0 + g.t;
      uint64_t v = 0;
      uint32_t nb = 0;
      if (k < ntok) {
        const uint32_t t = tok[k];
        if (t & CM_DF_TOK_LIT) {
          v = sh.ll_code[t & 0xffu];
          nb = sh.ll_len[t & 0xffu];
        } else {
          uint32_t nx, xv;
          const uint32_t ls = cm_df_len_sym(t >> 16, &nx, &xv);
          v = sh.ll_code[ls] | (uint64_t)xv << sh.ll_len[ls];
          nb = sh.ll_len[ls] + nx;
          const uint32_t ds = cm_df_dist_sym((t & 0xffffu) + 1u, &nx, &xv);
          v |= ((uint64_t)sh.d_code[ds] | (uint64_t)xv << sh.d_len[ds]) << nb;
          nb += sh.d_len[ds] + nx;
        }
      }
      uint32_t tot;
      const uint32_t o = g.scan(nb, &tot);
      cm_df_put(w, at + o, v, nb);
      at += tot;
    }
    if (g.t == 0) cm_df_put(w, at, sh.ll_code[256], sh.ll_len[256]);
    g.sync();
    for (uint32_t i = g.t; i < coded; i += G) out[18u + i] = win[i];
  } else {  // one stored block
    payload = n + 5u;
    if (g.t == 0) {
      out[18] = 1;
      out[19] = (uint8_t)(n & 0xffu);
      out[20] = (uint8_t)(n >> 8);
      out[21] = (uint8_t)(~n & 0xffu);
      out[22] = (uint8_t)((~n >> 8) & 0xffu);
    }
    for (uint32_t i = g.t; i < n; i += G) out[23u + i] = win[i];
  }
  const uint32_t total = 18u + payload + 8u;
  if (g.t == 0) {
    cm_df_bgzf_header(out, total);
    cm_df_bgzf_trailer(out + 18u + payload, crc, n);
  }
  g.sync();  // (the shared memory serves the group's next slice)
  return total;
}

#endif
