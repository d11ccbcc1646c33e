// cm_summary.h -- the per-barcode counters of --summary (SummaryMetadata, summary_metadata.h; fed by chromap.h:495-515, 1190-1230 and
// mapping_writer.h:281-350, 405-437) as an open-addressing table in HBM.  The device side is in this header so that the run-selection
// kernels of cm_post.hip and cm_sam_post.hip credit a run where they resolve it; the table itself lives in cm_summary.hip.
//
//   keys[cap]    2-bit packed (corrected) barcode; bulk data counts everything under key 0; CM_SM_EMPTY marks a free slot
//   first[cap]   smallest global read id that was counted under the key (TOTAL): the order in which the reference's hash map met the keys
//   cnt[4 * cap] TOTAL, DUP, LOWMAPQ, MAPPED
//   meta         [0] keys in the table, [1] raised when a key found no free slot, [2] TOTAL of the non-whitelist row, [3] slot of key 0
#ifndef CM_SUMMARY_H_
#define CM_SUMMARY_H_
#include <stdint.h>

#define CM_SM_EMPTY (~0ull)
#define CM_SM_TOTAL 0
#define CM_SM_DUP 1
#define CM_SM_LOWMAPQ 2
#define CM_SM_MAPPED 3
#define CM_SM_META_N 0
#define CM_SM_META_FULL 1
#define CM_SM_META_NONWL 2
#define CM_SM_META_SLOT0 3
#define CM_SM_META_WORDS 8

struct CmSmDev {  // keys == nullptr: the run has no summary -- the kernels do what they did without it
  unsigned long long *keys, *first;
  uint32_t *cnt, *meta;
  uint32_t mask;
  uint32_t slot0;  // slot of key 0, for runs whose records all count there (bulk data): one address for the whole grid
};

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t cm_sm_home(uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32); }

// slot of `key`, claimed when the key is new (linear probing; keys are never removed).  ~0u: no free slot, the flag is raised
__device__ __forceinline__ uint32_t cm_sm_slot(const CmSmDev &t, uint64_t key) {
  uint32_t b = cm_sm_home(key) & t.mask;
  for (uint32_t step = 0; step <= t.mask; ++step) {
    const unsigned long long k = t.keys[b];
    if (k == key) return b;
    if (k == CM_SM_EMPTY) {
      const unsigned long long old = atomicCAS(&t.keys[b], CM_SM_EMPTY, (unsigned long long)key);
      if (old == CM_SM_EMPTY) { atomicAdd(&t.meta[CM_SM_META_N], 1u); return b; }
      if (old == key) return b;
    }
    b = (b + 1) & t.mask;
  }
  atomicExch(&t.meta[CM_SM_META_FULL], 1u);
  return ~0u;
}

// A resolved run of d records under `key` (mapping_writer.h:281-301, 422-432): at or above the MAPQ threshold it has d - 1 duplicates,
// below it d low-MAPQ records; d mapped records either way.  one_key: every record of the launch counts under key 0 (slot0)
__device__ __forceinline__ void cm_sm_credit(const CmSmDev &t, bool one_key, uint64_t key, uint32_t d, bool pass) {
  const uint32_t s = one_key ? t.slot0 : cm_sm_slot(t, key);
  if (s == ~0u) return;
  uint32_t *c = t.cnt + 4ull * s;
  if (pass) { if (d > 1) atomicAdd(c + CM_SM_DUP, d - 1); }
  else atomicAdd(c + CM_SM_LOWMAPQ, d);
  atomicAdd(c + CM_SM_MAPPED, d);
}
#endif

struct cmgpu_ctx;
// the table for a kernel launch that may meet up to new_keys keys it does not hold yet -- or, total_bound != 0, whose run cannot hold
// more than total_bound keys at all (a whitelist) -- grown by rehash when it would pass half its slots; out->keys == nullptr when the
// context has no summary.  key0: also find / claim the slot of key 0 (out->slot0)
int cm_summary_dev(cmgpu_ctx *c, uint64_t new_keys, uint64_t total_bound, bool key0, CmSmDev *out);
// after the launches (the stream has been waited for): CMGPU_ECAPACITY when a key found no slot
int cm_summary_check(cmgpu_ctx *c);
// TOTAL of the resident batch, after its barcodes were corrected (cmgpu_map_resident)
int cm_summary_total(cmgpu_ctx *c);
#endif
