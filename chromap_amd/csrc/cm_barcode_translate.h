// cm_barcode_translate.h -- --barcode-translate (BarcodeTranslator, barcode_translator.h:42-101) for the device-side text writers
// (cm_post.hip: column 4 of the barcoded BED kinds; cm_sam_post.hip: the CB:Z: value) and for the host.
//
// The table's image (cmgpu_barcode_translation_pack builds it, cmgpu_set_barcode_translation uploads it):
//   buckets  2 x 64-bit words each: {key, to_offset << 32 | to_length}; a value word of all ones marks an empty bucket (every key
//            value is a legal key: 32 T's pack to all ones).  A power of two of them, at most half in use; a key lives in the first
//            free bucket from (key * CM_BT_HASH_MUL) >> 32 & mask onwards, with wrap-around -- the whitelist table's hash
//            (cm_post.hip: pp_abundance).  A probe step is ONE 16-byte load
//   blob     the `to` strings back to back, no terminators
// A barcode of bc_len bases is cut into bc_len / from_len segments with the reference's own shifts (:80-83), on 64-bit values -- not by
// characters: the two agree when bc_len is a multiple of from_len, and where it is not the shifts are what the reference prints.
// No segment (from_len > bc_len): the column is empty, as the reference's loop leaves it.
// No HIP header is needed: cm_host.cpp (also built by the host compiler alone) uses the same functions.
#ifndef CM_BARCODE_TRANSLATE_H_
#define CM_BARCODE_TRANSLATE_H_
#include <stdint.h>

#if defined(__HIPCC__)
#define CM_BT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define CM_BT_HD inline
#endif

#define CM_BT_HASH_MUL 0x9E3779B97F4A7C15ull
#define CM_BT_EMPTY (~0ull)

struct CmBtDev {
  const uint64_t *tab;  // nullptr: no table -- the writers print Seed2Sequence
  const uint8_t *blob;
  uint32_t mask, from_len;
};

CM_BT_HD void cm_bt_load(const uint64_t *tab, uint32_t b, uint64_t *key, uint64_t *val) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const u64x2 e = *reinterpret_cast<const u64x2 *>(tab + 2 * (uint64_t)b);  // global_load_dwordx4
  *key = e.x;
  *val = e.y;
#else
  *key = tab[2 * (uint64_t)b];
  *val = tab[2 * (uint64_t)b + 1];
#endif
}
// the value word of `seed`'s bucket; CM_BT_EMPTY: the table does not have it.  At most mask + 1 steps: an image without an empty
// bucket (the packer never makes one; a caller of cmgpu_barcode_translate_host may hand one in) ends the search as a miss
CM_BT_HD uint64_t cm_bt_find(const CmBtDev &t, uint64_t seed) {
  uint32_t b = (uint32_t)((seed * CM_BT_HASH_MUL) >> 32) & t.mask;
  for (uint32_t step = 0; step <= t.mask; ++step) {
    uint64_t k, v;
    cm_bt_load(t.tab, b, &k, &v);
    if (v == CM_BT_EMPTY || k == seed) return v;
    b = (b + 1) & t.mask;
  }
  return CM_BT_EMPTY;
}
// segment i of nseg = bc_len / from_len (nseg * from_len <= 32: no shift reaches 64)
CM_BT_HD uint64_t cm_bt_seed(const CmBtDev &t, uint64_t bc, uint32_t nseg, uint32_t i) {
  const uint64_t m = t.from_len >= 32 ? ~0ull : (1ull << (2 * t.from_len)) - 1;
  return ((bc << (2 * i * t.from_len)) >> (2 * (nseg - 1) * t.from_len)) & m;
}
// "length": bytes of to[0]-to[1]-...; false: a segment is not in the table
CM_BT_HD bool cm_bt_length(const CmBtDev &t, uint64_t bc, uint32_t bc_len, uint32_t *len) {
  const uint32_t nseg = bc_len / t.from_len;
  uint32_t l = nseg ? nseg - 1 : 0;
  for (uint32_t i = 0; i < nseg; ++i) {
    const uint64_t v = cm_bt_find(t, cm_bt_seed(t, bc, nseg, i));
    if (v == CM_BT_EMPTY) return false;
    l += (uint32_t)v;
  }
  *len = l;
  return true;
}
// "render": writes to[0]-to[1]-... at p, returns the byte after it (a segment that is not in the table writes nothing: the writers
// ask for the length first and print no line for such a barcode)
CM_BT_HD uint8_t *cm_bt_render(const CmBtDev &t, uint64_t bc, uint32_t bc_len, uint8_t *p) {
  const uint32_t nseg = bc_len / t.from_len;
  for (uint32_t i = 0; i < nseg; ++i) {
    if (i) *p++ = '-';
    const uint64_t v = cm_bt_find(t, cm_bt_seed(t, bc, nseg, i));
    if (v == CM_BT_EMPTY) continue;
    const uint8_t *s = t.blob + (v >> 32);
    const uint32_t l = (uint32_t)v;
    for (uint32_t k = 0; k < l; ++k) *p++ = s[k];
  }
  return p;
}
#endif
