// cm_summary.hip -- --summary on the device (cm_summary.h): the table, the TOTAL kernel, growth by rehash and the download.
// Replaces the per-batch TOTAL loop of the reference (chromap.h:495-515, 1190-1230); DUP / LOWMAPQ / MAPPED are credited by the
// run-selection kernels of cm_post.hip and cm_sam_post.hip.  The CSV itself is written on the host (cm_host.cpp: cmgpu_write_summary).
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "cm_ctx.h"
#include "cm_kernels.h"
#include "cm_summary.h"

#define SM_BLOCK 256
// TOTAL: one read (pair) per thread, counted under its corrected barcode key, under the non-whitelist row when CorrectBarcodeAt failed
// and such reads are not mapped (chromap.h:396-401, 1139-1142), under key 0 when the batch has no barcodes.  Equal keys are combined
// before the table is touched: inside a wave by comparing against the lowest uncounted lane's key (one step per distinct key), and
// across the block when each of its waves holds one and the same key -- bulk data then costs one atomic per block, and a cell's
// reads that stand together cost one per wave.  `first` takes the smallest global read id of the key.
__global__ __launch_bounds__(SM_BLOCK) void k_sm_total(CmSmDev t, const uint64_t *__restrict__ bc_key, const uint8_t *__restrict__ bc_ok, uint32_t n,
                                                         uint64_t first_read_id, int keep) {
  __shared__ unsigned long long s_key[SM_BLOCK / 64];
  __shared__ uint32_t s_cnt[SM_BLOCK / 64];
  __shared__ int s_one[SM_BLOCK / 64];
  const uint32_t i = blockIdx.x * SM_BLOCK + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool act = i < n;
  uint64_t key = 0;
  bool nonwl = false;
  if (act && bc_key) {
    key = bc_key[i];
    nonwl = !bc_ok[i] && !keep;
  }
  unsigned long long todo = __ballot(act);
  uint32_t my_cnt = 0, groups = 0;
  bool leader = false;
  while (todo) {
    const int l = __ffsll((long long)todo) - 1;
    const uint64_t lk = __shfl(key, l, 64);
    const int lnw = __shfl((int)nonwl, l, 64);
    const bool mine = act && key == lk && (int)nonwl == lnw;
    const unsigned long long m = __ballot(mine);
    if ((int)lane == l) { my_cnt = (uint32_t)__popcll(m); leader = true; }  // (the lowest lane of a group: its read id is the group's smallest)
    todo &= ~m;
    ++groups;
  }
  if (lane == 0) {
    s_one[wave] = act && groups == 1 && !nonwl && my_cnt == 64;
    s_key[wave] = key;
    s_cnt[wave] = my_cnt;
  }
  __syncthreads();
  bool block_one = true;
  uint32_t block_cnt = 0;
  for (uint32_t w = 0; w < SM_BLOCK / 64; ++w) {
    block_one = block_one && s_one[w] && s_key[w] == s_key[0];
    block_cnt += s_cnt[w];
  }
  uint32_t add = 0;
  if (block_one) { if (threadIdx.x == 0) add = block_cnt; }
  else if (leader) add = my_cnt;
  if (!add) return;
  if (nonwl) { atomicAdd(&t.meta[CM_SM_META_NONWL], add); return; }
  const uint32_t s = cm_sm_slot(t, key);
  if (s == ~0u) return;
  atomicAdd(t.cnt + 4ull * s + CM_SM_TOTAL, add);
  atomicMin(&t.first[s], (unsigned long long)(first_read_id + i));
}

// every key of the old table into the new one, with its counters and first read id (each key is moved by one thread)
__global__ __launch_bounds__(SM_BLOCK) void k_sm_rehash(CmSmDev o, CmSmDev t) {
  const uint32_t b = blockIdx.x * SM_BLOCK + threadIdx.x;
  if (b > o.mask) return;
  const unsigned long long k = o.keys[b];
  if (k == CM_SM_EMPTY) return;
  const uint32_t s = cm_sm_slot(t, k);
  if (s == ~0u) return;
  t.first[s] = o.first[b];
  for (int q = 0; q < 4; ++q) t.cnt[4ull * s + q] = o.cnt[4ull * b + q];
}
__global__ void k_sm_key0(CmSmDev t) { t.meta[CM_SM_META_SLOT0] = cm_sm_slot(t, 0); }
// slots in use -> dense {key, first, total, dup, lowmapq, mapped} entries (cmgpu_summary_entry)
__global__ __launch_bounds__(SM_BLOCK) void k_sm_gather(CmSmDev t, uint8_t *__restrict__ out, uint32_t *__restrict__ cursor, uint32_t capacity) {
  const uint32_t b = blockIdx.x * SM_BLOCK + threadIdx.x;
  if (b > t.mask) return;
  const unsigned long long k = t.keys[b];
  if (k == CM_SM_EMPTY) return;
  const uint32_t o = atomicAdd(cursor, 1u);
  if (o >= capacity) return;
  unsigned long long *e = reinterpret_cast<unsigned long long *>(out + (uint64_t)o * 32);
  const uint32_t *c = t.cnt + 4ull * b;
  e[0] = k;
  e[1] = t.first[b];
  e[2] = (unsigned long long)c[0] | ((unsigned long long)c[1] << 32);
  e[3] = (unsigned long long)c[2] | ((unsigned long long)c[3] << 32);
}

static void sm_view(const CmSummary &sm, CmSmDev *d) {
  d->keys = (unsigned long long *)sm.keys.p; d->first = (unsigned long long *)sm.first.p; d->cnt = (uint32_t *)sm.cnt.p; d->meta = (uint32_t *)sm.meta.p;
  d->mask = sm.cap - 1; d->slot0 = ~0u;
}
// an empty table of `cap` slots (a power of two) in sm; meta is cleared too
static int sm_alloc(cmgpu_ctx *c, CmSummary &sm, uint32_t cap) {
  if (sm.keys.ensure((size_t)cap * 8) || sm.first.ensure((size_t)cap * 8) || sm.cnt.ensure((size_t)cap * 16) || sm.meta.ensure(CM_SM_META_WORDS * 4)) {
    cm_set_error(c, "out of device memory (summary table of " + std::to_string(cap) + " slots)");
    return CMGPU_ENOMEM;
  }
  hipStream_t s = c->stream;
  CM_HIPCHECK(c, hipMemsetAsync(sm.keys.p, 0xff, (size_t)cap * 8, s));
  CM_HIPCHECK(c, hipMemsetAsync(sm.first.p, 0xff, (size_t)cap * 8, s));
  CM_HIPCHECK(c, hipMemsetAsync(sm.cnt.p, 0, (size_t)cap * 16, s));
  CM_HIPCHECK(c, hipMemsetAsync(sm.meta.p, 0, CM_SM_META_WORDS * 4, s));
  sm.cap = cap;
  sm.key_bound = 0;
  sm.slot0 = ~0u;
  return CMGPU_OK;
}
static uint32_t sm_pow2(uint64_t v) {
  uint64_t p = 1024;
  while (p < v) p <<= 1;
  return p > (1ull << 31) ? 0u : (uint32_t)p;
}

int cm_summary_dev(cmgpu_ctx *c, uint64_t new_keys, uint64_t total_bound, bool key0, CmSmDev *out) {
  memset(out, 0, sizeof(*out));
  CmSummary &sm = c->sm;
  if (!sm.on) return CMGPU_OK;
  hipStream_t s = c->stream;
  if (key0 && sm.slot0 == ~0u) ++new_keys;
  // The number of keys is bounded on the host: by the whitelist where it closes the key set, otherwise by what the launches so far could
  // have added.  Only when that bound would pass half the slots is the device's own count fetched -- a batch of a run with a closed
  // whitelist, and nearly every batch of any other run, starts its kernel without a round trip.
  uint64_t want;
  if (total_bound) {
    if (sm.key_bound < total_bound) sm.key_bound = total_bound;
    want = sm.key_bound + 1;  // (+ key 0, which records without a barcode count under)
  } else {
    if (2 * (sm.key_bound + new_keys + 1) > sm.cap) {
      uint32_t k = 0;
      CM_HIPCHECK(c, hipMemcpyAsync(&k, (uint32_t *)sm.meta.p + CM_SM_META_N, 4, hipMemcpyDeviceToHost, s));
      CM_HIPCHECK(c, cm_stream_sync(s));
      sm.key_bound = k;
    }
    want = sm.key_bound + new_keys + 1;
  }
  if (2 * want > sm.cap) {  // the table stays at most half full: grown to fit (and once more, so that the next batches fit too), keys and counters re-inserted
    uint32_t cap = total_bound ? 0u : sm_pow2(4 * want);
    if (!cap) cap = sm_pow2(2 * want);
    if (!cap) { cm_set_error(c, "summary: more than 2^30 distinct barcodes"); return CMGPU_ECAPACITY; }
    CmSummary old = sm;
    sm.keys = DevBuf(); sm.first = DevBuf(); sm.cnt = DevBuf(); sm.meta = DevBuf();
    int rc = sm_alloc(c, sm, cap);
    if (rc) { sm.keys.release(); sm.first.release(); sm.cnt.release(); sm.meta.release(); sm = old; return rc; }
    CmSmDev o, t;
    sm_view(old, &o);
    sm_view(sm, &t);
    hipLaunchKernelGGL(k_sm_rehash, dim3((old.cap + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, s, o, t);
    // (the non-whitelist counter and the flag move as they are; the number of keys was counted again by the insertions)
    CM_HIPCHECK(c, hipMemcpyAsync((uint32_t *)sm.meta.p + 1, (uint32_t *)old.meta.p + 1, 2 * 4, hipMemcpyDeviceToDevice, s));
    CM_HIPCHECK(c, cm_stream_sync(s));
    old.keys.release(); old.first.release(); old.cnt.release(); old.meta.release();
    sm.key_bound = old.key_bound;  // (sm_alloc started the new table's bound at 0; the slot of key 0 is another one now)
  }
  if (!total_bound) sm.key_bound += new_keys;
  sm_view(sm, out);
  if (key0) {
    if (sm.slot0 == ~0u) {
      hipLaunchKernelGGL(k_sm_key0, dim3(1), dim3(1), 0, s, *out);
      CM_HIPCHECK(c, hipMemcpyAsync(&sm.slot0, (uint32_t *)sm.meta.p + CM_SM_META_SLOT0, 4, hipMemcpyDeviceToHost, s));
      CM_HIPCHECK(c, cm_stream_sync(s));
    }
    out->slot0 = sm.slot0;
  }
  return CMGPU_OK;
}

int cm_summary_check(cmgpu_ctx *c) {
  if (!c->sm.on) return CMGPU_OK;
  uint32_t full = 0;  // (on the context's stream: a copy on the null stream would wait for the ingest's streams too)
  CM_HIPCHECK(c, hipMemcpyAsync(&full, (uint32_t *)c->sm.meta.p + CM_SM_META_FULL, 4, hipMemcpyDeviceToHost, c->stream));
  CM_HIPCHECK(c, cm_stream_sync(c->stream));
  if (full) { cm_set_error(c, "summary: the barcode table ran out of slots; its counts are incomplete"); return CMGPU_ECAPACITY; }
  return CMGPU_OK;
}

int cm_summary_total(cmgpu_ctx *c) {
  if (!c->sm.on || c->n_pairs == 0) return CMGPU_OK;
  if (c->has_barcodes && c->bc_len >= 32) { cm_set_error(c, "summary: barcodes of 32 bases are not supported"); return CMGPU_EINVAL; }
  const uint32_t n = c->n_pairs;
  // keys this batch can add: with a whitelist and unlisted reads left out, the whitelist bounds the whole run; otherwise every read may
  // bring its own
  const bool closed = c->has_barcodes && c->wl_size && !c->p.bc_keep;
  CmSmDev t;
  int rc = cm_summary_dev(c, c->has_barcodes ? (uint64_t)n : 1, closed ? (uint64_t)c->wl_size : 0, false, &t);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sm_total, dim3((n + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, c->stream, t,
                     c->has_barcodes ? (const uint64_t *)c->bc_key.p : (const uint64_t *)nullptr,
                     c->has_barcodes ? (const uint8_t *)c->bc_ok.p : (const uint8_t *)nullptr, n, (uint64_t)c->first_read_id, c->p.bc_keep);
  // (waited for, because the ingest's streams may refill the barcode keys once the call returns.  The flag of a full table is looked at
  //  where the table is read -- cmgpu_summary_download and the format calls: the table is grown before it can fill)
  CM_HIPCHECK(c, cm_stream_sync(c->stream));
  return CMGPU_OK;
}

extern "C" int cmgpu_summary_enable(cmgpu_ctx *c, int on) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  CmSummary &sm = c->sm;
  if (!on) { sm.on = false; return CMGPU_OK; }
  if (sm.on) return CMGPU_OK;
  // sized from the whitelist where there is one (every key of a run without --output-mappings-not-in-whitelist is on it)
  const uint32_t cap = sm_pow2(2 * ((uint64_t)c->wl_size + 1));
  const int rc = sm_alloc(c, sm, cap);
  if (rc) return rc;
  CM_HIPCHECK(c, cm_stream_sync(c->stream));
  sm.on = true;
  return CMGPU_OK;
}

extern "C" int cmgpu_summary_clear(cmgpu_ctx *c) {
  if (!c) return CMGPU_EINVAL;
  if (!c->sm.on) return CMGPU_OK;
  CM_HIPCHECK(c, cm_enter(c));
  const int rc = sm_alloc(c, c->sm, c->sm.cap);
  if (rc) return rc;
  CM_HIPCHECK(c, cm_stream_sync(c->stream));
  return CMGPU_OK;
}

extern "C" int cmgpu_summary_info(cmgpu_ctx *c, uint64_t *n_keys, uint64_t *n_slots) {
  if (!c) return CMGPU_EINVAL;
  if (n_keys) *n_keys = 0;
  if (n_slots) *n_slots = 0;
  if (!c->sm.on) return CMGPU_OK;
  CM_HIPCHECK(c, cm_enter(c));
  uint32_t k = 0;
  CM_HIPCHECK(c, hipMemcpyAsync(&k, (uint32_t *)c->sm.meta.p + CM_SM_META_N, 4, hipMemcpyDeviceToHost, c->stream));
  CM_HIPCHECK(c, cm_stream_sync(c->stream));
  if (n_keys) *n_keys = k;
  if (n_slots) *n_slots = c->sm.cap;
  return CMGPU_OK;
}

extern "C" int cmgpu_summary_download(cmgpu_ctx *c, cmgpu_summary_entry *out, uint64_t capacity, uint64_t *n_out, uint64_t *nonwhitelist_total) {
  if (!c || !n_out || (!out && capacity)) return CMGPU_EINVAL;
  *n_out = 0;
  if (nonwhitelist_total) *nonwhitelist_total = 0;
  if (!c->sm.on) { cm_set_error(c, "the context has no summary (cmgpu_summary_enable)"); return CMGPU_EINVAL; }
  CM_HIPCHECK(c, cm_enter(c));
  { const int rc = cm_summary_check(c); if (rc) return rc; }
  uint32_t meta[CM_SM_META_WORDS];
  CM_HIPCHECK(c, hipMemcpyAsync(meta, c->sm.meta.p, sizeof(meta), hipMemcpyDeviceToHost, c->stream));
  CM_HIPCHECK(c, cm_stream_sync(c->stream));
  const uint32_t k = meta[CM_SM_META_N];
  if (nonwhitelist_total) *nonwhitelist_total = meta[CM_SM_META_NONWL];
  if (k > capacity) { *n_out = k; cm_set_error(c, "summary buffer too small"); return CMGPU_ECAPACITY; }
  if (k) {
    DevBuf dense, cursor;
    if (dense.ensure((size_t)k * 32) || cursor.ensure(4)) { dense.release(); cursor.release(); cm_set_error(c, "out of device memory (summary download)"); return CMGPU_ENOMEM; }
    CmSmDev t;
    sm_view(c->sm, &t);
    hipError_t e = hipMemsetAsync(cursor.p, 0, 4, c->stream);
    hipLaunchKernelGGL(k_sm_gather, dim3((c->sm.cap + SM_BLOCK - 1) / SM_BLOCK), dim3(SM_BLOCK), 0, c->stream, t, (uint8_t *)dense.p, (uint32_t *)cursor.p, k);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dense.p, (size_t)k * 32, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = cm_stream_sync(c->stream);
    dense.release(); cursor.release();
    if (e != hipSuccess) { cm_set_error(c, std::string("summary download: ") + hipGetErrorString(e)); return CMGPU_EHIP; }
  }
  *n_out = k;
  return CMGPU_OK;
}
