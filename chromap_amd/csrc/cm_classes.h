// cm_classes.h -- the size-class policy of the long-list stages: which list lengths go to a lane, a group of 16 lanes, a wave or a
// block (the table in cm_types.h).  The classes' fixed sizes; the sizes that follow from options, batch and device, computed once per
// pair range (cm_size_classes; cm_api.hip); and a function per stage that sends a list length to a CmList id or CM_L_NONE -- the kernels
// call these and keep no threshold of their own.  Plain arithmetic, no HIP header: tests/hostemu compiles it with g++
// (tests/test_hostemu_classes.py, tests/test_class_dispatch_cpu.py).  The classes decide who works on a list, never the result.
#ifndef CM_CLASSES_H_
#define CM_CLASSES_H_
#include "cm_types.h"

// ---- the fixed sizes.  *_COOP_MIN: the longest list that stays with its lane; *_P_*: entries of a class's shared work area
#define CM_RS_COOP_MIN 32u    // rescue hits on a strand
#define CM_S4B_PMAX 7680u     // rescue hits the largest shared work area holds (20 bytes per hit: 8192 would pass the CU's 160 KB)
#define CM_S4C_COOP_MIN 48u   // pair filter: entries of a merged candidate list
#define CM_S4C_P_SMALL 256u   // most pairs with long lists: a wave each (the classes above take a block of 256 lanes per pair)
#define CM_S4C_P_WAVE 1024u   // entries of a candidate list the work arrays of a wave hold
#define CM_S4C_P_BLOCK 4096u  // ... of a block
#define CM_S4C_P_BIG 15360u   // ... of a block of 1024 lanes that leaves the position lists in global memory (a lane walking such a
                              // pair's two-pointer loop at global latency was the whole 16 ms of k_s4c_reduce on the mosaic genome)
#define CM_S5C_COOP_MIN 48u   // candidates of a read above which S5 (sorting the lists, alignments, acceptance) is a wave's work
#define CM_S5C_P_SMALL 512u   // most reads of the wave class: work arrays of this size (more waves per CU)
#define CM_S5C_P_WAVE 2048u   // candidates of a strand the wave's work arrays hold
#define CM_S5C_P_BLOCK 16384u // ... a block's (longer lists: the acceptance loop by one lane)
#define CM_S6A_COOP_MIN 48u   // pairing (S6a and S6c): draft mappings of a read and strand
#define CM_S6A_P_SMALL 256u
#define CM_S6A_P_WAVE 1024u
#define CM_S6A_P_BLOCK 8192u

struct CmClassIn {
  // cmgpu_set_option: heavy_wave_max / heavy_block_max / heavy_big_max, heavy_mid_max, s3b_lane_cap (0: the defaults below)
  int heavy_max[3];
  int heavy_mid;
  int s3b_cap;
  uint32_t max_read_len;  // of the resident batch
  uint32_t n_seq;         // reference sequences
  bool has_goff;          // CmDev::goff exists: the cooperative hit-list kernel works on 32-bit keys
  uint32_t lane_cap;      // cm_s3b_lane_cap(max_read_len)
  uint32_t hv_max[4], hv_big;  // cm_s3b_heavy_classes: the kernels' own classes (hv_big 0: the device refused the large LDS allocation)
};

// -> d.hv_max, hv_big, rs_max3, rs_big, hv_mid, hv_sub, s3b_cap
static inline void cm_size_classes(const CmClassIn &in, CmDev &d) {
  d.s3b_cap = in.s3b_cap > 0 ? (uint32_t)in.s3b_cap : in.lane_cap;
  d.hv_max[0] = d.hv_max[1] = d.hv_max[2] = d.hv_max[3] = 0;
  d.hv_big = d.rs_max3 = d.rs_big = d.hv_mid = d.hv_sub = 0;
  if (in.n_seq >= 0x80000000u) return;  // the cooperative kernel keeps the strand in bit 31 of the sequence id: no classes
  for (int q = 0; q < 4; ++q) d.hv_max[q] = in.hv_max[q];
  d.hv_big = in.hv_big;
  // tests force the classes: heavy_wave_max caps the wave class, heavy_block_max the two middle classes, heavy_big_max the largest
  if (in.heavy_max[0] > 0 && (uint32_t)in.heavy_max[0] < d.hv_max[0]) d.hv_max[0] = (uint32_t)in.heavy_max[0];
  for (int q = 1; q <= 2; ++q) if (in.heavy_max[1] > 0 && (uint32_t)in.heavy_max[1] < d.hv_max[q]) d.hv_max[q] = (uint32_t)in.heavy_max[1];
  if (in.heavy_max[2] > 0 && (uint32_t)in.heavy_max[2] < d.hv_max[3]) d.hv_max[3] = (uint32_t)in.heavy_max[2];
  for (int q = 1; q < 4; ++q) if (d.hv_max[q] < d.hv_max[q - 1]) d.hv_max[q] = d.hv_max[q - 1];
  if (in.heavy_max[2] > 0 && (uint32_t)in.heavy_max[2] < d.hv_big) d.hv_big = (uint32_t)in.heavy_max[2];
  const uint32_t hv_big_area = d.hv_big;  // (what a CU's shared memory holds once: the rescue lists' largest class is sized from it)
  // 32-bit hit keys: 11 bytes per hit -- 7 040 hits leave room for TWO blocks of 1 024 lanes per CU (k_s3b_coop<1024, true> on profile 2:
  // 53.6 -> 43.0 ms of S3b per step against one block with 8 192; the few longer lists go to the slab launch)
  if (in.has_goff && d.hv_big > 7040u) d.hv_big = 7040u;
  if (d.hv_big <= d.hv_max[3]) d.hv_big = 0;
  if (in.heavy_max[0] < 0) { d.hv_max[0] = d.hv_max[1] = d.hv_max[2] = d.hv_max[3] = 0; d.hv_big = 0; }  // everything long goes to the one-lane path
  // the rescue lists' classes: the hit lists' up to 2048, then as many 20-byte entries as fit a CU's shared memory twice / once
  d.rs_max3 = d.hv_max[3] < 3968u ? d.hv_max[3] : 3968u;
  // (round 6, measured and NOT kept: 32-bit keys in k_s4b_coop as in k_s3b_coop -- 12 instead of 20 bytes per entry, classes of 6 400 / 3 968
  //  entries at two / three blocks per CU.  The stage got SLOWER, profile 2 46.5 -> 49.7 ms and profile 1 9.7 -> 18.3 ms per step: unlike the
  //  hit lists, the rescue lists are merged with the read's own candidates and written back as sequence << 32 | position, so every hit
  //  pays a lookup of its sequence's offset on the way in and every candidate a search of the offset table on the way out, and the
  //  groups' time is not the number of reads in flight here)
  d.rs_big = d.hv_big ? (hv_big_area < CM_S4B_PMAX ? hv_big_area : CM_S4B_PMAX) : 0u;
  if (d.rs_big <= d.rs_max3) d.rs_big = 0;
  // the longest list a 16-lane group takes: 64 hits; 96 for reads of 100 bases and more (round 6, `tools/gpu_mid_knob.sh`: 2 x 150 hic reads
  // carry ~37 hits each with a tail to ~100 -- 64 / 80 / 96 / 112: 102.6 / 101.8 / 110.3 / 101.3 M pairs/s, twice; at 50 bases 96 is neutral on the
  // headline and the mammalian-like genomes and loses 4 % on the planted repeats)
  d.hv_mid = in.heavy_mid < 0 ? 0u : (in.heavy_mid > 0 ? (uint32_t)in.heavy_mid : (in.max_read_len >= 100 ? 96u : 64u));
  if (d.hv_mid > 256) d.hv_mid = 256;
  if (d.hv_max[0] == 0) d.hv_mid = 0;
  d.hv_sub = d.hv_max[0] >= 512 ? 256u : 0u;  // (the tests' small size classes: no sub-class)
  // with the 16-lane groups taking the lists up to hv_mid, a lane keeps the short ones only (16 hits: 256-thread blocks)
  if (d.hv_mid && in.s3b_cap <= 0 && d.s3b_cap > 16) d.s3b_cap = 16;
}

// ---- a length -> the list of its class.  Hit lists (k_s3a_count): the hits of a read
CM_HD uint32_t cm_hit_class(const CmDev &d, uint32_t tot) {
  return tot <= d.s3b_cap ? CM_L_NONE /* the lane's own slots */ : tot <= d.hv_mid ? CM_L_HIT_G16 : tot <= d.hv_sub ? CM_L_HIT_WAVE_SMALL : tot <= d.hv_max[0] ? CM_L_HIT_WAVE
         : tot <= d.hv_max[1] ? CM_L_HIT_B256A : tot <= d.hv_max[2] ? CM_L_HIT_B256B : tot <= d.hv_max[3] ? CM_L_HIT_B512 : tot <= d.hv_big ? CM_L_HIT_B1024 : CM_L_HIT_SLAB;
}
// rescue lists (S4b): the longer of a read's two lists of rescue hits; what no slab holds stays with a lane
CM_HD uint32_t cm_rescue_class(const CmDev &d, uint32_t big) {
  if (big <= CM_RS_COOP_MIN || d.hv_max[0] == 0) return CM_L_NONE;
  return big <= d.hv_max[0] ? CM_L_RS_WAVE : big <= d.hv_max[1] ? CM_L_RS_B256A : big <= d.hv_max[2] ? CM_L_RS_B256B : big <= d.rs_max3 ? CM_L_RS_B512 : big <= d.rs_big ? CM_L_RS_B1024
         : (d.coop_slab && big <= d.coop_slab_cap) ? CM_L_RS_SLAB : CM_L_NONE;
}
// pair filter (S4c): the longest of the pair's four merged candidate lists
CM_HD uint32_t cm_pf_class(const CmDev &d, uint32_t big) {
  if (big <= CM_S4C_COOP_MIN) return CM_L_NONE;
  return big <= CM_S4C_P_SMALL ? CM_L_PF_WAVE : big <= CM_S4C_P_WAVE ? CM_L_PF_BLOCK : big <= CM_S4C_P_BLOCK ? CM_L_PF_BLOCK_BIG : big <= d.s4c_pbig ? CM_L_PF_HUGE : CM_L_NONE;
}
// verification (S5): a read's filtered candidates on the + and the - strand
CM_HD uint32_t cm_s5_class(uint32_t fcp, uint32_t fcn) {
  if (fcp + fcn <= CM_S5C_COOP_MIN) return CM_L_NONE;
  const uint32_t big = fcp > fcn ? fcp : fcn;
  return big <= CM_S5C_P_SMALL ? CM_L_S5_SMALL : big <= CM_S5C_P_WAVE ? CM_L_S5_WAVE : CM_L_S5_BLOCK;
}
// pairing: the longest of the pair's four lists of draft mappings decides whether a group works, the longer list of read 2 (the one
// it stages) which; the small / wave / block list are the caller's -- S6a's or S6c's
CM_HD uint32_t cm_s6_class(uint32_t big, uint32_t big2, uint32_t small_list, uint32_t wave_list, uint32_t block_list) {
  if (big <= CM_S6A_COOP_MIN) return CM_L_NONE;
  return big2 <= CM_S6A_P_SMALL ? small_list : big2 <= CM_S6A_P_WAVE ? wave_list : block_list;
}
#endif
