// cm_post.hip -- device-side post-processing of the mapping records:
// what MappingProcessor::SortOutputMappings / RemovePCRDuplicate (mapping_processor.h:100-202),
// the low-memory merge (mapping_writer.h:166-376) and the BED writers (mapping_writer.cc:44-131)
// do on the host, as radix sorts + one selection pass + one text-formatting pass in HBM.
//
//   record store   dense cmgpu_record array (+ parallel barcode array) that batches append to
//   sort           LSD over 64-bit key words, payload = record index:
//                    w0 = mapq | direction | is_unique | read_id            (40 bits)
//                    [w1 = barcode]                                          (single-cell only)
//                    wT = rid | fragment_start | fragment_length            (48 + rid bits)
//                  == per-rid std::sort with the record's operator< (bed_mapping.h:32-38,
//                  85-90, 145-153, 208-215); read_id is unique, so later tie fields never decide
//   select         one thread per sorted position: head of an operator== run picks the run's
//                  survivor (low-memory merge: first record with the maximal MAPQ; in-memory
//                  RemovePCRDuplicate: last record of the run), num_dups = min(255, run length),
//                  MAPQ filter, line length
//   format         exclusive scan of line lengths; each block renders its lines into LDS and
//                  stores them with coalesced writes
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <cstring>

#include <condition_variable>
#include <mutex>
#include <thread>
#include <rocprim/rocprim.hpp>

#include <chrono>
#include <vector>

#include "cm_alloc.h"
#include "cm_ctx.h"
#include "cm_kernels.h"
#include "cm_summary.h"
#include "cm_text_job.h"

#define PP_RUN_SERIAL 128u  // records of a duplicate run its head walks alone (k_pp_select); longer runs: k_pp_select_long
#define PP_BLOCK 256
#define PP_LDS_BYTES 32768
#define PP_LEN_MISS (~0ull)  // allocation only: a survivor whose barcode the translation table lacks, until k_al_apply knows whether it is printed

struct PpCfg {
  int kind;       // CMGPU_TEXT_BED_PE / _SE / _PE_BC
  int dedup;      // remove_pcr_duplicates
  int inmem;      // !low_memory_mode: Tn5 shift before the sort, last-of-run survives
  int tn5;
  int mapq_thr;
  uint32_t n_seq;
  uint32_t bc_len;
  int bulk;       // single-cell data, duplicate removal at bulk level (mapping_writer.h:202-345)
  int last_section;   // this store ends the output (always, unless a higher rank of a multi-GPU run owns records too)
  const uint64_t *wl;  // whitelist table {key, abundance} (cm_api.hip: cmgpu_set_whitelist), linear probing
  uint32_t wl_mask;
  CmBtDev bt;          // --barcode-translate: column 4 of the barcoded BED kinds through the table (bt.tab == nullptr: Seed2Sequence)
  unsigned long long *bt_miss;  // surviving lines whose barcode the table does not have (the job's spare count word)
  int alloc;           // --allocate-multi-mappings (in-memory flavour): the selection leaves the MAPQ filter to k_al_apply
};

struct PpRec {  // cmgpu_record, read with two 8-byte loads + one 8-byte load
  uint32_t read_id, rid, start;
  uint16_t len;
  uint8_t mapq, dir, uniq, dups;
  uint16_t pal, nal;
};

__device__ __forceinline__ PpRec pp_load(const uint8_t *store, uint32_t i) {
  const uint64_t *p = reinterpret_cast<const uint64_t *>(store + (uint64_t)i * 24);
  const uint64_t a = p[0], b = p[1], c = p[2];
  PpRec r;
  r.read_id = (uint32_t)a;
  r.rid = (uint32_t)(a >> 32);
  r.start = (uint32_t)b;
  r.len = (uint16_t)(b >> 32);
  r.mapq = (uint8_t)(b >> 48);
  r.dir = (uint8_t)(b >> 56);
  r.uniq = (uint8_t)c;
  r.dups = (uint8_t)(c >> 8);
  r.pal = (uint16_t)(c >> 16);
  r.nal = (uint16_t)(c >> 32);
  return r;
}

__host__ __device__ __forceinline__ bool pp_se_bc(int kind) { return kind == CMGPU_TEXT_BED_SE_BC || kind == CMGPU_TEXT_TAGALIGN_SE_BC; }
__host__ __device__ __forceinline__ bool pp_has_bc(int kind) { return kind == CMGPU_TEXT_BED_PE_BC || kind == CMGPU_TEXT_TAGALIGN_PE_BC || pp_se_bc(kind); }
__host__ __device__ __forceinline__ bool pp_prints_bc(int kind) { return kind == CMGPU_TEXT_BED_PE_BC || kind == CMGPU_TEXT_BED_SE_BC; }
__host__ __device__ __forceinline__ bool pp_is_se(int kind) { return kind == CMGPU_TEXT_BED_SE || pp_se_bc(kind); }
__host__ __device__ __forceinline__ bool pp_tagalign(int kind) { return kind == CMGPU_TEXT_TAGALIGN_PE || kind == CMGPU_TEXT_TAGALIGN_PE_BC; }
// Tn5Shift (bed_mapping.h:48-54, 100-106, 165-170, 224-229)
__device__ __forceinline__ void pp_tn5(PpRec &r, int kind) {
  if (pp_is_se(kind)) {
    if (r.dir == 1) r.start += 4; else r.len = (uint16_t)(r.len - 5);
  } else {
    r.start += 4;
    r.len = (uint16_t)(r.len - 9);
    r.pal = (uint16_t)(r.pal - 4);
    r.nal = (uint16_t)(r.nal - 5);
  }
}

__global__ __launch_bounds__(PP_BLOCK) void k_pp_key0(const uint8_t *__restrict__ store, uint32_t n, uint64_t *__restrict__ key,
                                                        uint32_t *__restrict__ idx) {
  const uint32_t i = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const PpRec r = pp_load(store, i);
  key[i] = ((uint64_t)(r.mapq & 63) << 34) | ((uint64_t)(r.dir & 1) << 33) | ((uint64_t)(r.uniq & 1) << 32) | r.read_id;
  idx[i] = i;
}

__global__ __launch_bounds__(PP_BLOCK) void k_pp_key_bc(const uint64_t *__restrict__ bc, const uint32_t *__restrict__ idx, uint32_t n,
                                                          uint64_t *__restrict__ key) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j < n) key[j] = bc[idx[j]];
}

// which = 0: (rid[low 16] , start, len); which = 1: rid >> 16 (only when n_seq > 65536)
__global__ __launch_bounds__(PP_BLOCK) void k_pp_key_top(const uint8_t *__restrict__ store, const uint32_t *__restrict__ idx, uint32_t n,
                                                           PpCfg cfg, int which, uint64_t *__restrict__ key) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j >= n) return;
  PpRec r = pp_load(store, idx[j]);
  if (cfg.inmem && cfg.tn5) pp_tn5(r, cfg.kind);
  key[j] = which == 0 ? ((uint64_t)(r.rid & 0xffff) << 48) | ((uint64_t)r.start << 16) | r.len : (uint64_t)(r.rid >> 16);
}

__device__ __forceinline__ bool pp_same_run(const PpRec &a, uint64_t bca, const PpRec &b, uint64_t bcb, const PpCfg &cfg) {
  if (a.rid != b.rid || a.start != b.start) return false;
  if (cfg.kind == CMGPU_TEXT_BED_SE) return true;          // bed_mapping.h:91-94
  if (pp_se_bc(cfg.kind)) return bca == bcb;               // MappingWithBarcode: (barcode, start), :39-42
  if (a.len != b.len) return false;                        // :216-219
  return !pp_has_bc(cfg.kind) || bca == bcb;               // :154-159
}

__device__ __forceinline__ uint32_t pp_abundance(const PpCfg &cfg, uint64_t key) {
  const uint64_t x = key * 0x9E3779B97F4A7C15ull;
  uint32_t b = (uint32_t)(x >> 32) & cfg.wl_mask;
  for (;;) {
    const uint64_t k = cfg.wl[2 * (uint64_t)b];
    if (k == key) return (uint32_t)cfg.wl[2 * (uint64_t)b + 1];
    if (k == ~0ull) return 0;
    b = (b + 1) & cfg.wl_mask;
  }
}

// --summary: a resolved run of `dups` records whose survivor (barcode bcv) has MAPQ `mapq` (mapping_writer.h:281-301; the in-memory
// writer counts the survivor's num_dups_, capped at 255, :420-432)
__device__ __forceinline__ void pp_sm_run(const CmSmDev &sm, const PpCfg &cfg, uint64_t bcv, uint32_t dups, uint32_t mapq) {
  if (cfg.inmem && dups > 255) dups = 255;
  cm_sm_credit(sm, !pp_has_bc(cfg.kind), bcv, dups, (int)mapq >= cfg.mapq_thr);
}

// the survivor of sorted position j: MAPQ filter, Tn5 shift, line length; win / dups / line_len of the position.  bcv: the survivor's
// barcode.  With a translation table a barcode it does not have is counted, for a line that would be printed only (the reference
// exits in Translate, which it calls for a mapping it is about to print)
__device__ __forceinline__ void pp_finish(uint32_t j, PpRec r, uint32_t wi, uint64_t bcv, uint32_t dups, bool bulk_done, const PpCfg &cfg,
                                          const uint32_t *__restrict__ name_off, uint32_t *__restrict__ win,
                                          uint32_t *__restrict__ dups_out, uint64_t *__restrict__ line_len) {
  if ((!bulk_done && !cfg.alloc && (int)r.mapq < cfg.mapq_thr) || r.rid >= cfg.n_seq) { line_len[j] = 0; return; }
  if (cfg.tn5) pp_tn5(r, cfg.kind);
  if (dups > 255) dups = 255;
  const uint32_t nm = name_off[r.rid + 1] - name_off[r.rid];
  uint32_t len;
  if (pp_tagalign(cfg.kind)) {
    // two lines (mapping_writer.cc:84-117, 138-168): the + read's and the - read's alignment; bulk data
    // prints num_dups on the second line, single-cell data prints neither barcode nor num_dups
    const uint32_t pe = r.start + r.pal, ne = r.start + r.len, ns = ne - r.nal;
    len = 2 * (nm + 1 + 2 + cm_digits10(r.mapq) + 1 + 1 + 1) + cm_digits10(r.start) + 1 + cm_digits10(pe) + 1 + cm_digits10(ns) + 1 + cm_digits10(ne) + 1;
    if (cfg.kind == CMGPU_TEXT_TAGALIGN_PE) len += 1 + cm_digits10(dups);
  } else {
    len = nm + 1 + cm_digits10(r.start) + 1 + cm_digits10(r.start + r.len) + 1;
    if (pp_prints_bc(cfg.kind)) {  // chr start end barcode dups
      uint32_t bl = cfg.bc_len;
      if (cfg.bt.tab && !cm_bt_length(cfg.bt, bcv, cfg.bc_len, &bl)) {
        if (cfg.alloc) { win[j] = wi; dups_out[j] = dups; line_len[j] = PP_LEN_MISS; return; }
        atomicAdd(cfg.bt_miss, 1ull); line_len[j] = 0; return;
      }
      len += bl + 1 + cm_digits10(dups) + 1;
    }
    else if (cfg.kind == CMGPU_TEXT_TAGALIGN_SE_BC) len += 2 + cm_digits10(r.mapq) + 2 + 1;     // chr start end N mapq strand (mapping_writer.cc:26-34)
    else len += 2 + cm_digits10(r.mapq) + 3 + cm_digits10(dups) + 1;                              // chr start end N mapq strand dups
  }
  win[j] = wi;
  dups_out[j] = dups;
  line_len[j] = len;
}

// survivor index (into the store), num_dups and line length per sorted position (0 = no line)
__global__ __launch_bounds__(PP_BLOCK) void k_pp_select(const uint8_t *__restrict__ store, const uint64_t *__restrict__ bc,
                                                          const uint32_t *__restrict__ idx, uint32_t n, PpCfg cfg,
                                                          const uint32_t *__restrict__ name_off, uint32_t *__restrict__ win,
                                                          uint32_t *__restrict__ dups_out, uint64_t *__restrict__ line_len,
                                                          uint32_t *__restrict__ long_list, uint32_t *__restrict__ long_cnt, CmSmDev sm) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j >= n) return;
  uint32_t wi = idx[j];
  PpRec r = pp_load(store, wi);
  const uint64_t rbc = pp_has_bc(cfg.kind) ? bc[wi] : 0;
  PpRec rs = r;  // the run identity is evaluated on what was sorted (shifted first in in-memory mode)
  if (cfg.inmem && cfg.tn5) pp_tn5(rs, cfg.kind);
  uint32_t dups = 1;
  bool bulk_done = false;
  if (cfg.dedup && cfg.bulk) {
    // bulk-level runs: same (rid, start, length) whatever the barcode; barcode groups are consecutive.
    // A group is represented by its last record and weighs 1 (single record) or 2 (any larger group);
    // FindBestMappingIndexFromDuplicates: larger weight, then larger abundance, first on ties.
    if (j > 0) {
      PpRec p = pp_load(store, idx[j - 1]);
      if (p.rid == r.rid && p.start == r.start && (pp_is_se(cfg.kind) || p.len == r.len)) { line_len[j] = 0; return; }
    }
    uint32_t t = j, best_i = wi, best_nd = 0, best_ab = 0, maxq_mapq = r.mapq;
    bool have = false;
    while (t < n) {
      if (t > j + PP_RUN_SERIAL) {  // a pile-up: the barcode groups of the run by a wave (k_pp_select_long)
        long_list[atomicAdd(long_cnt, 1u)] = j;
        line_len[j] = 0;
        return;
      }
      const uint32_t gi = idx[t];
      const PpRec gr = pp_load(store, gi);
      if (gr.rid != r.rid || gr.start != r.start || (!pp_is_se(cfg.kind) && gr.len != r.len)) break;
      const uint64_t gb = bc[gi];
      uint32_t u = t + 1, rep = gi, gsize = 1;
      if (gr.mapq > maxq_mapq) maxq_mapq = gr.mapq;
      while (u < n) {
        const uint32_t qi = idx[u];
        const PpRec q = pp_load(store, qi);
        if (q.rid != r.rid || q.start != r.start || (!pp_is_se(cfg.kind) && q.len != r.len) || bc[qi] != gb) break;
        if (q.mapq > maxq_mapq) maxq_mapq = q.mapq;
        rep = qi;
        ++gsize;
        ++u;
        if (u > j + PP_RUN_SERIAL) {  // one cell's pile-up at one position (10^4 .. 10^5 duplicates): the wave kernel's too
          long_list[atomicAdd(long_cnt, 1u)] = j;
          line_len[j] = 0;
          return;
        }
      }
      const uint32_t nd = gsize >= 2 ? 2u : 1u, ab = pp_abundance(cfg, gb);
      if (!have || nd > best_nd || (nd == best_nd && ab > best_ab)) { have = true; best_i = rep; best_nd = nd; best_ab = ab; }
      t = u;
    }
    dups = t - j;
    wi = best_i;
    r = pp_load(store, wi);
    // the very last run of the output is filtered on the run's maximal MAPQ (mapping_writer.h:331-337)
    const uint32_t filter_mapq = t == n && cfg.last_section ? maxq_mapq : (uint32_t)r.mapq;
    // (the output's last run is tested before the best barcode group is chosen, mapping_writer.h:323-350: when it fails, the counts go
    //  to the record the merge held then -- the first one of the run's largest MAPQ)
    if (sm.keys && r.rid < cfg.n_seq) {
      uint32_t ci = wi;
      if ((int)filter_mapq < cfg.mapq_thr && t == n && cfg.last_section)
        for (uint32_t u = j; u < t; ++u) { ci = idx[u]; if (pp_load(store, ci).mapq == maxq_mapq) break; }
      pp_sm_run(sm, cfg, bc[ci], dups, filter_mapq);
    }
    if ((int)filter_mapq < cfg.mapq_thr) { line_len[j] = 0; return; }
    bulk_done = true;
  } else
  if (cfg.dedup) {
    if (j > 0) {
      const uint32_t pi = idx[j - 1];
      PpRec p = pp_load(store, pi);
      if (cfg.inmem && cfg.tn5) pp_tn5(p, cfg.kind);
      if (pp_same_run(p, pp_has_bc(cfg.kind) ? bc[pi] : 0, rs, rbc, cfg)) { line_len[j] = 0; return; }
    }
    uint32_t t = j + 1;
    bool ended = false;
    for (; t < n && t <= j + PP_RUN_SERIAL; ++t) {
      const uint32_t qi = idx[t];
      PpRec q = pp_load(store, qi), qs = q;
      if (cfg.inmem && cfg.tn5) pp_tn5(qs, cfg.kind);
      if (!pp_same_run(rs, rbc, qs, pp_has_bc(cfg.kind) ? bc[qi] : 0, cfg)) { ended = true; break; }
      ++dups;
      if (cfg.inmem || q.mapq > r.mapq) { r = q; wi = qi; }
    }
    if (!ended && t < n) {  // a pile-up (PCR duplicates at a hot spot run to 10^5 records): a wave takes the run, k_pp_select_long
      long_list[atomicAdd(long_cnt, 1u)] = j;
      line_len[j] = 0;
      return;
    }
  }
  if (sm.keys && !bulk_done && r.rid < cfg.n_seq) pp_sm_run(sm, cfg, pp_has_bc(cfg.kind) ? bc[wi] : 0, dups, r.mapq);
  pp_finish(j, r, wi, cfg.bt.tab ? bc[wi] : 0, dups, bulk_done, cfg, name_off, win, dups_out, line_len);
}

// Duplicate runs longer than PP_RUN_SERIAL, one wave each: the lanes test 64 records per step for membership (the run is the
// contiguous prefix of members), keep the first record of maximal MAPQ (low-memory rule: a later record replaces the survivor
// only with a strictly larger MAPQ, mapping_writer.h:252-262) or the run's last record (in-memory rule), and lane 0 finishes
// the position as k_pp_select does.  Bulk-level de-duplication of single-cell data (barcode groups inside a run): the first branch.
__global__ __launch_bounds__(64) void k_pp_select_long(const uint8_t *__restrict__ store, const uint64_t *__restrict__ bc,
                                                       const uint32_t *__restrict__ idx, uint32_t n, PpCfg cfg,
                                                       const uint32_t *__restrict__ name_off, uint32_t *__restrict__ win,
                                                       uint32_t *__restrict__ dups_out, uint64_t *__restrict__ line_len,
                                                       const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ long_cnt, CmSmDev sm) {
  const uint32_t lane = threadIdx.x, cnt = *long_cnt;
  for (uint32_t e = blockIdx.x; e < cnt; e += gridDim.x) {
    const uint32_t j = long_list[e];
    const uint32_t wi0 = idx[j];
    const PpRec r0 = pp_load(store, wi0);
    if (cfg.dedup && cfg.bulk) {
      // Bulk-level duplicate removal of single-cell data (mapping_writer.h:126-163, 202-345) for a long run: the records with the
      // run's (rid, start, length) in steps of 64; barcode groups are consecutive; a group is represented by its LAST record and
      // weighs 2 (two records or more) or 1; the survivor is the group of largest (weight, abundance of its barcode), the first one
      // on ties.  The lane that holds a group's last record knows the group's size (its first record: the nearest group start at or
      // before it in this step, or the start carried over from earlier steps) and proposes it; the proposals are reduced per step.
      unsigned long long best_key = 0;  // weight << 32 | abundance, + 1 so that 0 means none
      uint32_t best_pos = 0, maxq = r0.mapq, run_end = n, carried_start = j;
      for (uint32_t base = j; base < n; base += 64) {
        const uint32_t t = base + lane;
        bool mem = false, next_same = false;
        uint64_t gb = 0;
        uint32_t qm = 0;
        if (t < n) {
          const uint32_t qi = idx[t];
          const PpRec q = pp_load(store, qi);
          mem = q.rid == r0.rid && q.start == r0.start && (pp_is_se(cfg.kind) || q.len == r0.len);
          gb = bc[qi];
          qm = q.mapq;
          if (mem && t + 1 < n) {
            const uint32_t ni = idx[t + 1];
            const PpRec nq = pp_load(store, ni);
            next_same = nq.rid == r0.rid && nq.start == r0.start && (pp_is_se(cfg.kind) || nq.len == r0.len) && bc[ni] == gb;
          }
        }
        const unsigned long long mm = __ballot(mem);
        const uint32_t pre = mm == ~0ull ? 64u : (uint32_t)(__ffsll((long long)~mm) - 1);  // members before the first non-member
        const bool in = lane < pre;
        // group starts in this step: the run's first record, or a barcode that differs from the previous record's
        const uint64_t pb = __shfl_up(gb, 1, 64);
        const bool first = in && (t == j || (lane > 0 ? pb != gb : false));
        // (lane 0 of a later step: its predecessor is the previous step's lane 63, whose next_same said whether the group goes on)
        unsigned long long fm = __ballot(first);
        const bool last = in && !next_same;
        uint32_t gstart = carried_start;
        const unsigned long long below = fm & ((lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull)));
        if (below) gstart = base + (63u - (uint32_t)__clzll((long long)below));
        if (in && qm > maxq) maxq = qm;
        unsigned long long key = 0;
        if (last) {
          const uint32_t gsize = t - gstart + 1;
          key = (((unsigned long long)(gsize >= 2 ? 2u : 1u) << 32) | pp_abundance(cfg, gb)) + 1ull;
        }
        uint32_t pos = t;
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned long long ok = __shfl_down(key, off, 64);
          const uint32_t op = __shfl_down(pos, off, 64);
          const uint32_t om = __shfl_down(maxq, off, 64);
          if (ok > key || (ok == key && ok && op < pos)) { key = ok; pos = op; }
          if (om > maxq) maxq = om;
        }
        key = __shfl(key, 0, 64); pos = __shfl(pos, 0, 64); maxq = __shfl(maxq, 0, 64);
        if (key > best_key) { best_key = key; best_pos = pos; }  // (an equal key of a later step: the earlier group stays)
        // the group that runs over the end of this step started at: its start in this step, or further back
        {
          const unsigned long long lastm = __ballot(last);
          const bool open = pre == 64 && !((lastm >> 63) & 1ull);  // lane 63's record is a member and its group goes on
          if (open && fm) carried_start = base + (63u - (uint32_t)__clzll((long long)fm));
          // (open without a start in this step: the carried start stays; not open: the next step's lane 0 starts a group itself)
          if (!open) carried_start = base + 64;
        }
        if (pre < 64) { run_end = base + pre; break; }
      }
      if (lane == 0) {
        const uint32_t wi = idx[best_pos];
        const PpRec r = pp_load(store, wi);
        const uint32_t filter_mapq = run_end == n && cfg.last_section ? maxq : (uint32_t)r.mapq;
        if (sm.keys && r.rid < cfg.n_seq) {
          uint32_t ci = wi;
          if ((int)filter_mapq < cfg.mapq_thr && run_end == n && cfg.last_section)  // (k_pp_select: the first record of the run's largest MAPQ)
            for (uint32_t t = j; t < run_end; ++t) { ci = idx[t]; if (pp_load(store, ci).mapq == maxq) break; }
          pp_sm_run(sm, cfg, bc[ci], run_end - j, filter_mapq);
        }
        if ((int)filter_mapq < cfg.mapq_thr) line_len[j] = 0;
        else pp_finish(j, r, wi, cfg.bt.tab ? bc[wi] : 0, run_end - j, true, cfg, name_off, win, dups_out, line_len);
      }
      continue;
    }
    const uint64_t rbc = pp_has_bc(cfg.kind) ? bc[wi0] : 0;
    PpRec rs = r0;
    if (cfg.inmem && cfg.tn5) pp_tn5(rs, cfg.kind);
    int my_mapq = -1;
    uint32_t my_pos = ~0u, run_end = n;
    for (uint32_t base = j + 1; base < n; base += 64) {
      const uint32_t t = base + lane;
      bool same = false;
      int qm = -1;
      if (t < n) {
        const uint32_t qi = idx[t];
        PpRec q = pp_load(store, qi), qs = q;
        if (cfg.inmem && cfg.tn5) pp_tn5(qs, cfg.kind);
        same = pp_same_run(rs, rbc, qs, pp_has_bc(cfg.kind) ? bc[qi] : 0, cfg);
        qm = (int)q.mapq;
      }
      const unsigned long long m = __ballot(same);
      const uint32_t pre = m == ~0ull ? 64u : (uint32_t)(__ffsll((long long)~m) - 1);  // members before the first non-member
      if (lane < pre && qm > my_mapq) { my_mapq = qm; my_pos = t; }
      if (pre < 64) { run_end = base + pre; break; }
    }
    // first record of maximal MAPQ over the lanes
    for (int off = 32; off > 0; off >>= 1) {
      const int om = __shfl_down(my_mapq, off, 64);
      const uint32_t op = __shfl_down(my_pos, off, 64);
      if (om > my_mapq || (om == my_mapq && op < my_pos)) { my_mapq = om; my_pos = op; }
    }
    if (lane == 0) {
      PpRec r = r0;
      uint32_t wi = wi0;
      if (cfg.inmem) { wi = idx[run_end - 1]; r = pp_load(store, wi); }
      else if (my_mapq > (int)r0.mapq) { wi = idx[my_pos]; r = pp_load(store, wi); }
      if (sm.keys && r.rid < cfg.n_seq) pp_sm_run(sm, cfg, pp_has_bc(cfg.kind) ? bc[wi] : 0, run_end - j, r.mapq);
      pp_finish(j, r, wi, cfg.bt.tab ? bc[wi] : 0, run_end - j, false, cfg, name_off, win, dups_out, line_len);
    }
  }
}

// ---------------------------------------------------------------------------------------
// --allocate-multi-mappings (MappingProcessor::AllocateMultiMappings, mapping_processor.h:319-440), between the selection and the
// line offsets.  In allocation mode the selection keeps every survivor of duplicate removal (line length != 0) whatever its MAPQ:
//   classify   survivor with MAPQ >= 4: uni-mapping, below: multi-mapping; one 64-bit word per position (uni count low, multi count
//              high), so that one exclusive scan numbers both
//   scatter    uni-mappings: (rid << 32 | start) -- ascending already, the positions are sorted by (rid, start, length) -- and
//              (rid << 32 | end), radix-sorted next; multi-mappings: sorted position and read_id, then stable-sorted by read_id, which
//              leaves a read's members in (chromosome rank, position) order as std::stable_sort(ReadIdLess) does
//   weight     one thread per multi-mapping, in group order: #(start < interval_end) - #(end <= interval_start) by two binary searches
//              over the whole arrays (the chromosomes below the query's cancel out); end <= interval_start implies start <
//              interval_end, so the difference is the reference's interval-tree count.  No atomics
//   group      heads from the sorted read_ids; a scan by key gives every read's weight sum at its last member, where the reads
//              with and without overlaps are counted
//   draw       on the host (cm_alloc.h) over the downloaded weights; the kept members' numbers come back
//   apply      every multi-mapping that was not kept, and every survivor below the MAPQ threshold, loses its line
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ PpRec al_survivor(const uint8_t *store, const uint32_t *__restrict__ win, uint32_t j, const PpCfg &cfg) {
  PpRec r = pp_load(store, win[j]);
  if (cfg.tn5) pp_tn5(r, cfg.kind);  // (in-memory flavour: the coordinates that were sorted)
  return r;
}

__global__ __launch_bounds__(PP_BLOCK) void k_al_classify(const uint8_t *__restrict__ store, const uint32_t *__restrict__ win,
                                                            const uint64_t *__restrict__ line_len, uint32_t n, uint64_t *__restrict__ cls) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j > n) return;
  uint64_t v = 0;
  if (j < n && line_len[j]) v = pp_load(store, win[j]).mapq >= CM_ALLOC_MIN_UNIQUE_MAPQ ? 1ull : 1ull << 32;
  cls[j] = v;  // (cls[n] = 0: the scan's last element is the two totals)
}

__global__ __launch_bounds__(PP_BLOCK) void k_al_scatter(const uint8_t *__restrict__ store, const uint32_t *__restrict__ win,
                                                           const uint64_t *__restrict__ cls, const uint64_t *__restrict__ cls_off, uint32_t n,
                                                           PpCfg cfg, uint64_t *__restrict__ uni_start, uint64_t *__restrict__ uni_end,
                                                           uint32_t *__restrict__ multi_pos, uint32_t *__restrict__ multi_read,
                                                           uint32_t *__restrict__ multi_num) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint64_t v = cls[j];
  if (!v) return;
  const PpRec r = al_survivor(store, win, j, cfg);
  const uint64_t off = cls_off[j];
  if (v == 1ull) {
    const uint32_t u = (uint32_t)off;
    uni_start[u] = ((uint64_t)r.rid << 32) | r.start;
    uni_end[u] = ((uint64_t)r.rid << 32) | (uint32_t)(r.start + r.len);
  } else {
    const uint32_t m = (uint32_t)(off >> 32);
    multi_pos[m] = j;
    multi_read[m] = r.read_id;
    multi_num[m] = m;
  }
}

// first index in a[0 .. n) whose element is >= key (upper: > key)
__device__ __forceinline__ uint32_t al_bound(const uint64_t *__restrict__ a, uint32_t n, uint64_t key, bool upper) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t v = a[mid];
    if (upper ? v <= key : v < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(PP_BLOCK) void k_al_weight(const uint8_t *__restrict__ store, const uint32_t *__restrict__ win, PpCfg cfg,
                                                          const uint64_t *__restrict__ uni_start, const uint64_t *__restrict__ uni_end,
                                                          uint32_t n_uni, const uint32_t *__restrict__ multi_pos,
                                                          const uint32_t *__restrict__ group_read, const uint32_t *__restrict__ group_num,
                                                          uint32_t n_multi, int distance, uint32_t *__restrict__ weight,
                                                          uint32_t *__restrict__ weight_head) {
  const uint32_t g = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (g >= n_multi) return;
  const PpRec r = al_survivor(store, win, multi_pos[group_num[g]], cfg);
  const uint32_t start = r.start, end = r.start + r.len;
  const uint32_t qs = start > (uint32_t)distance ? start - (uint32_t)distance : 0;  // mapping_processor.h:270-275
  const uint32_t qe = end + (uint32_t)distance;
  const uint32_t a = al_bound(uni_start, n_uni, ((uint64_t)r.rid << 32) | qe, false);
  const uint32_t b = al_bound(uni_end, n_uni, ((uint64_t)r.rid << 32) | qs, true);
  const uint32_t w = a > b ? a - b : 0;
  const bool head = g == 0 || group_read[g - 1] != group_read[g];
  weight[g] = w;
  weight_head[g] = w | (head ? CM_ALLOC_HEAD : 0u);
}

// sum[g]: inclusive sum of the weights of g's read up to g.  cnt[0]: reads whose weights sum to more than 0, cnt[1]: to 0
__global__ __launch_bounds__(PP_BLOCK) void k_al_count(const uint32_t *__restrict__ group_read, const uint32_t *__restrict__ sum,
                                                         uint32_t n_multi, unsigned long long *__restrict__ cnt) {
  const uint32_t g = blockIdx.x * PP_BLOCK + threadIdx.x;
  const bool tail = g < n_multi && (g + 1 == n_multi || group_read[g + 1] != group_read[g]);
  const bool some = tail && sum[g] != 0;
  const unsigned long long ms = __ballot(some), mz = __ballot(tail && !some);
  if ((threadIdx.x & 63u) == 0) {
    if (ms) atomicAdd(cnt, (unsigned long long)__popcll(ms));
    if (mz) atomicAdd(cnt + 1, (unsigned long long)__popcll(mz));
  }
}

__global__ __launch_bounds__(PP_BLOCK) void k_al_mark(const uint32_t *__restrict__ kept, uint32_t n_kept, const uint32_t *__restrict__ group_num,
                                                        const uint32_t *__restrict__ multi_pos, uint32_t n_multi, uint32_t n,
                                                        uint8_t *__restrict__ keep) {
  const uint32_t k = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (k >= n_kept) return;
  const uint32_t g = kept[k];
  if (g >= n_multi) return;
  const uint32_t j = multi_pos[group_num[g]];
  if (j < n) keep[j] = 1;
}

__global__ __launch_bounds__(PP_BLOCK) void k_al_apply(const uint8_t *__restrict__ store, const uint32_t *__restrict__ win,
                                                         const uint8_t *__restrict__ keep, uint32_t n, PpCfg cfg, uint64_t *__restrict__ line_len) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint64_t ll = line_len[j];
  if (!ll) return;
  const uint32_t mapq = pp_load(store, win[j]).mapq;
  if ((mapq < CM_ALLOC_MIN_UNIQUE_MAPQ && !keep[j]) || (int)mapq < cfg.mapq_thr) { line_len[j] = 0; return; }
  if (ll == PP_LEN_MISS) { atomicAdd(cfg.bt_miss, 1ull); line_len[j] = 0; }  // a printed line whose barcode the table lacks
}

// leave_bc (translated barcodes only): room is left for column 4 instead of writing it, and the column's place is returned -- the
// block's waves fill it in (pp_fill_columns).  line_len: the line's bytes, from which the column's end follows without a lookup
__device__ __forceinline__ uint8_t *pp_render(uint8_t *p, const PpRec &r, uint64_t bcv, uint32_t dups, const PpCfg &cfg,
                                              const uint8_t *__restrict__ names, const uint32_t *__restrict__ name_off, bool leave_bc,
                                              uint32_t line_len) {
  uint8_t *col = nullptr;
  uint8_t *const line = p;
  const uint32_t n0 = name_off[r.rid], n1 = name_off[r.rid + 1];
  if (pp_tagalign(cfg.kind)) {
    const uint32_t pe = r.start + r.pal, ne = r.start + r.len, ns = ne - r.nal;
    for (int half = 0; half < 2; ++half) {
      const bool plus = (half == 0) == (r.dir != 0);  // the + read's line comes first when read 1 is on the + strand
      for (uint32_t i = n0; i < n1; ++i) *p++ = names[i];
      *p++ = '\t';
      p = cm_put_u32(p, plus ? r.start : ns);
      *p++ = '\t';
      p = cm_put_u32(p, plus ? pe : ne);
      *p++ = '\t'; *p++ = 'N'; *p++ = '\t';
      p = cm_put_u32(p, r.mapq);
      *p++ = '\t';
      *p++ = plus ? '+' : '-';
      if (half == 1 && cfg.kind == CMGPU_TEXT_TAGALIGN_PE) { *p++ = '\t'; p = cm_put_u32(p, dups); }
      *p++ = '\n';
    }
    return col;
  }
  for (uint32_t i = n0; i < n1; ++i) *p++ = names[i];
  *p++ = '\t';
  p = cm_put_u32(p, r.start);
  *p++ = '\t';
  p = cm_put_u32(p, r.start + r.len);
  *p++ = '\t';
  if (pp_prints_bc(cfg.kind)) {
    if (!cfg.bt.tab) {
      for (uint32_t b = 0; b < cfg.bc_len; ++b) *p++ = "ACGT"[(bcv >> ((cfg.bc_len - 1 - b) * 2)) & 3];  // Seed2Sequence
    } else if (leave_bc) {
      col = p;
      p = line + line_len - (1 + cm_digits10(dups) + 1);  // what follows the column: tab, dups, newline
    } else {
      p = cm_bt_render(cfg.bt, bcv, cfg.bc_len, p);
    }
    *p++ = '\t';
  } else {
    *p++ = 'N';
    *p++ = '\t';
    p = cm_put_u32(p, r.mapq);
    *p++ = '\t';
    *p++ = r.dir ? '+' : '-';
    if (cfg.kind == CMGPU_TEXT_TAGALIGN_SE_BC) { *p = '\n'; return col; }
    *p++ = '\t';
  }
  p = cm_put_u32(p, dups);
  *p = '\n';
  return col;
}

// A block whose lines do not fit the LDS staging (translated names of a few hundred bytes) writes them to the text directly.  The
// fixed columns are a few bytes per line and stay with the line's lane; the translated barcode is the bulk of such a line, and a
// lane that copied it alone would issue one single-byte store per byte, each lane of the wave to a different line.  Instead every
// wave takes its 64 lines one after the other and all lanes copy the line's `to` strings, consecutive bytes to consecutive lanes
// (the SAM writer's lanes-per-line copy, cm_sam_post.hip: sp_copy, without its word-wide middle: the strings start anywhere).
// col: where this lane's line left room for the column (nullptr: no line); every lane of the block calls this
__device__ __forceinline__ void pp_fill_columns(uint8_t *col, uint64_t bcv, const PpCfg &cfg) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nseg = cfg.bc_len / cfg.bt.from_len;
  for (unsigned long long m = __ballot(col != nullptr); m; m &= m - 1) {
    const int src = __ffsll((long long)m) - 1;
    uint8_t *d = reinterpret_cast<uint8_t *>(__shfl((unsigned long long)(uintptr_t)col, src, 64));
    const uint64_t key = __shfl((unsigned long long)bcv, src, 64);
    for (uint32_t i = 0; i < nseg; ++i) {
      if (i) { if (lane == 0) *d = '-'; ++d; }
      const uint64_t v = cm_bt_find(cfg.bt, cm_bt_seed(cfg.bt, key, nseg, i));  // (the same bucket for every lane: one request)
      if (v == CM_BT_EMPTY) continue;
      const uint8_t *s = cfg.bt.blob + (v >> 32);
      const uint32_t l = (uint32_t)v;
      for (uint32_t t = lane; t < l; t += 64) d[t] = s[t];
      d += l;
    }
  }
}

__global__ __launch_bounds__(PP_BLOCK) void k_pp_format(const uint8_t *__restrict__ store, const uint64_t *__restrict__ bc,
                                                          const uint32_t *__restrict__ win, const uint32_t *__restrict__ dups,
                                                          const uint64_t *__restrict__ line_len, const uint64_t *__restrict__ line_off,
                                                          uint32_t n, PpCfg cfg, const uint8_t *__restrict__ names,
                                                          const uint32_t *__restrict__ name_off, uint8_t *__restrict__ text) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[PP_LDS_BYTES];
  const uint32_t j0 = blockIdx.x * PP_BLOCK, j = j0 + threadIdx.x;
  const uint32_t jend = j0 + PP_BLOCK < n ? j0 + PP_BLOCK : n;
  const uint64_t base = line_off[j0], total = line_off[jend] - base;
  const bool staged = total <= PP_LDS_BYTES;
  const bool by_waves = !staged && cfg.bt.tab != nullptr;  // (the whole block's)
  uint8_t *col = nullptr;
  uint64_t bcv = 0;
  if (j < n && line_len[j]) {
    PpRec r = pp_load(store, win[j]);
    if (cfg.tn5) pp_tn5(r, cfg.kind);
    const uint64_t off = line_off[j];
    bcv = pp_has_bc(cfg.kind) ? bc[win[j]] : 0;
    col = pp_render(staged ? lds + (off - base) : text + off, r, bcv, dups[j], cfg, names, name_off, by_waves, (uint32_t)line_len[j]);
  }
  if (by_waves) pp_fill_columns(col, bcv, cfg);
  if (!staged) return;
  __syncthreads();
  // coalesced copy LDS -> text: bytes up to the first 16-byte boundary, aligned body, tail
  uint8_t *dst = text + base;
  const uint32_t tot = (uint32_t)total;
  uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
  if (head > tot) head = tot;
  for (uint32_t i = threadIdx.x; i < head; i += PP_BLOCK) dst[i] = lds[i];
  const uint32_t body = (tot - head) >> 4;
  for (uint32_t q = threadIdx.x; q < body; q += PP_BLOCK) {
    const uint8_t *s = lds + head + (q << 4);
    uint32_t w[4];
    for (int k = 0; k < 4; ++k)
      w[k] = (uint32_t)s[4 * k] | ((uint32_t)s[4 * k + 1] << 8) | ((uint32_t)s[4 * k + 2] << 16) | ((uint32_t)s[4 * k + 3] << 24);
    *reinterpret_cast<uint4 *>(dst + head + (q << 4)) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  for (uint32_t i = head + (body << 4) + threadIdx.x; i < tot; i += PP_BLOCK) dst[i] = lds[i];
}

// the valid record slots, dense (cm_compact_records): slot i goes to position pos[i] unless that is past the destination's cap records
__global__ void k_pp_compact(const uint8_t *__restrict__ rec, const uint8_t *__restrict__ ok, const uint32_t *__restrict__ pos,
                             const uint64_t *__restrict__ bc_in, uint8_t *__restrict__ dst, uint64_t *__restrict__ bc_dst, uint32_t n,
                             uint32_t per_pair, uint64_t cap) {  // per_pair record slots share one barcode key
  const uint32_t i = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (i >= n || !ok[i]) return;
  const uint32_t o = pos[i];
  if (o >= cap) return;
  const uint64_t *s = reinterpret_cast<const uint64_t *>(rec + (uint64_t)i * 24);
  uint64_t *d = reinterpret_cast<uint64_t *>(dst + (uint64_t)o * 24);
  d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
  if (bc_dst) bc_dst[o] = bc_in[i / per_pair];
}
__global__ void k_pp_flag(const uint8_t *ok, uint32_t *flag, uint32_t n) {
  const uint32_t i = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (i < n) flag[i] = ok[i];
}
__global__ void k_pp_split_bc(const uint8_t *__restrict__ in32, uint32_t n, uint8_t *__restrict__ dst, uint64_t *__restrict__ bc_dst) {
  const uint32_t i = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t *s = reinterpret_cast<const uint64_t *>(in32 + (uint64_t)i * 32);
  uint64_t *d = reinterpret_cast<uint64_t *>(dst + (uint64_t)i * 24);
  d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
  bc_dst[i] = s[3];
}

// ---------------------------------------------------------------------------------------
// record store
// ---------------------------------------------------------------------------------------
int cm_store_reserve(cmgpu_ctx *c, uint64_t need, bool with_bc) {
  if (need > 0xfffffff0ull) { cm_set_error(c, "record store is limited to 2^32 records"); return CMGPU_ECAPACITY; }
  if (need > c->store_cap) {
    uint64_t cap = c->store_cap ? c->store_cap * 2 : 1u << 20;
    if (cap < need) cap = need;
    CmTmpBuf nb, nbc;
    if (nb.ensure(cap * 24 + 16) || ((with_bc || c->store_has_bc) && nbc.ensure(cap * 8))) {
      cm_set_error(c, "out of device memory (record store)");
      return CMGPU_ENOMEM;
    }
    if (c->store_n) {
      CM_HIPCHECK(c, hipMemcpy(nb.p, c->store.p, c->store_n * 24, hipMemcpyDeviceToDevice));
      if (c->store_has_bc) CM_HIPCHECK(c, hipMemcpy(nbc.p, c->store_bc.p, c->store_n * 8, hipMemcpyDeviceToDevice));
    }
    c->store.release(); c->store_bc.release();
    c->store = nb.hand_over(); c->store_bc = nbc.hand_over();
    c->store_cap = cap;
  } else if (with_bc && !c->store_bc.p) {
    if (c->store_bc.ensure(c->store_cap * 8)) { cm_set_error(c, "out of device memory (record store)"); return CMGPU_ENOMEM; }
  }
  if (with_bc) c->store_has_bc = true;
  return CMGPU_OK;
}

// room for n_records in the store ahead of time (a run knows roughly how many pairs it will map: growing the store on
// demand doubles it with an allocation, a device-to-device copy and a synchronous free each time)
extern "C" int cmgpu_store_reserve(cmgpu_ctx *c, uint64_t n_records, int barcoded) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  { const int qrc = cm_exchange_quiesce(c); if (qrc) return qrc; }
  if (c->store_n && c->store_has_bc != (barcoded != 0)) { cm_set_error(c, "record store mixes barcoded and bulk batches"); return CMGPU_EINVAL; }
  const bool had_bc = c->store_has_bc;
  const int rc = cm_store_reserve(c, n_records, barcoded != 0);
  if (c->store_n == 0) c->store_has_bc = had_bc;  // an empty store takes the kind of the first append
  return rc;
}

extern "C" int cmgpu_store_clear(cmgpu_ctx *c) {
  if (!c) return CMGPU_EINVAL;
  (void)cm_exchange_quiesce(c);
  c->store_n = 0;
  c->store_has_bc = false;
  c->store_pairs_rec = false;
  c->text_bytes = 0;
  c->text_lines = 0;
  c->bam_starts_have = false;
  return CMGPU_OK;
}

extern "C" int cmgpu_store_append_resident(cmgpu_ctx *c, uint64_t *n_total) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  { const int qrc = cm_exchange_quiesce(c); if (qrc) return qrc; }
  const uint32_t n = (uint32_t)cm_rec_slots(c);
  if (c->store_n && c->store_has_bc != c->has_barcodes) { cm_set_error(c, "record store mixes barcoded and bulk batches"); return CMGPU_EINVAL; }
  if (n) {
    if (cm_store_kind_mismatch(c, cm_pairs_records(c))) return CMGPU_EINVAL;
    if (c->store_n == 0) c->store_pairs_rec = cm_pairs_records(c);
    int rc = cm_store_reserve(c, c->store_n + n, c->has_barcodes);
    if (rc) return rc;
    const uint32_t *n_valid = nullptr;
    rc = cm_compact_records(c, (uint8_t *)c->store.p + c->store_n * 24, c->has_barcodes ? (uint64_t *)c->store_bc.p + c->store_n : (uint64_t *)nullptr,
                            n, c->stream, &n_valid);
    if (rc) return rc;
    uint32_t k = 0;
    CM_HIPCHECK(c, hipMemcpyAsync(&k, n_valid, 4, hipMemcpyDeviceToHost, c->stream));
    CM_HIPCHECK(c, cm_stream_sync(c->stream));
    c->store_n += k;
  }
  if (n_total) *n_total = c->store_n;
  return CMGPU_OK;
}

extern "C" int cmgpu_store_append(cmgpu_ctx *c, const void *records, uint64_t n, int on_device, int barcoded) {
  if (!c || (!records && n)) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  { const int qrc = cm_exchange_quiesce(c); if (qrc) return qrc; }
  if (c->store_n && c->store_has_bc != (barcoded != 0)) { cm_set_error(c, "record store mixes barcoded and bulk batches"); return CMGPU_EINVAL; }
  if (n == 0) return CMGPU_OK;
  // the caller's records are of the kind the context's batches have (cmgpu_download_records hands out no other)
  if (cm_store_kind_mismatch(c, cm_pairs_records(c))) return CMGPU_EINVAL;
  if (c->store_n == 0) c->store_pairs_rec = cm_pairs_records(c);
  int rc = cm_store_reserve(c, c->store_n + n, barcoded != 0);
  if (rc) return rc;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (!barcoded) {
    CM_HIPCHECK(c, hipMemcpy((uint8_t *)c->store.p + c->store_n * 24, records, n * 24, kind));
  } else {
    CmTmpBuf tmp;
    const void *src = records;
    if (!on_device) {
      if (tmp.ensure(n * 32)) { cm_set_error(c, "out of device memory (record staging)"); return CMGPU_ENOMEM; }
      CM_HIPCHECK(c, hipMemcpy(tmp.p, records, n * 32, hipMemcpyHostToDevice));
      src = tmp.p;
    }
    cm_store_split_bc(c, src, n, c->stream);
    CM_HIPCHECK(c, cm_stream_sync(c->stream));
  }
  c->store_n += n;
  return CMGPU_OK;
}

// the allocation stage of cmgpu_store_format: after the selection kernels, before the line offsets.  job.loff is free until scan_lines and
// takes the classification's scan
static int pp_allocate(cmgpu_ctx *c, CmTextJob &job, const PpCfg &cfg, const cmgpu_params *p, const uint8_t *store, const uint32_t *win, uint32_t n) {
  hipStream_t s = c->stream;
  const dim3 b(PP_BLOCK), g((n + PP_BLOCK - 1) / PP_BLOCK), g1(n / PP_BLOCK + 1);
  CmTmpBuf cls, keep, tmp;
  if (cls.ensure(((size_t)n + 1) * 8) || keep.ensure((size_t)n)) return job.enomem("allocation");
  CM_HIPCHECK(c, hipMemsetAsync(keep.p, 0, (size_t)n, s));
  uint64_t *cls_off = (uint64_t *)job.loff.p;
  hipLaunchKernelGGL(k_al_classify, g1, b, 0, s, store, win, (const uint64_t *)job.llen.p, n, (uint64_t *)cls.p);
  { const int rc = cm_scan_u64(c, (const uint64_t *)cls.p, cls_off, (size_t)n + 1, tmp, s, "allocation scan"); if (rc) return rc; }
  uint64_t totals = 0;
  CM_HIPCHECK(c, hipMemcpyAsync(&totals, cls_off + n, 8, hipMemcpyDeviceToHost, s));
  CM_HIPCHECK(c, cm_stream_sync(s));
  const uint32_t n_uni = (uint32_t)totals, n_multi = (uint32_t)(totals >> 32);
  c->alloc_multi = n_multi;
  if (n_uni >= CM_ALLOC_HEAD) { cm_set_error(c, "allocation is limited to 2^31 uni-mappings"); return CMGPU_ECAPACITY; }
  if (n_multi) {  // (none: the reference asserts; here the text is the plain one)
    const dim3 gm((n_multi + PP_BLOCK - 1) / PP_BLOCK);
    CmTmpBuf us, ue0, ue1, mpos, mread0, mread1, mnum0, mnum1, wt, wh, sum, cnt, kept_d;
    const size_t ub = ((size_t)n_uni + 1) * 8, mb = (size_t)n_multi * 4;
    if (us.ensure(ub) || ue0.ensure(ub) || ue1.ensure(ub) || mpos.ensure(mb) || mread0.ensure(mb) || mread1.ensure(mb) || mnum0.ensure(mb) ||
        mnum1.ensure(mb) || wt.ensure(mb) || wh.ensure(mb) || sum.ensure(mb) || cnt.ensure(16)) return job.enomem("allocation");
    CM_HIPCHECK(c, hipMemsetAsync(cnt.p, 0, 16, s));
    hipLaunchKernelGGL(k_al_scatter, g, b, 0, s, store, win, (const uint64_t *)cls.p, (const uint64_t *)cls_off, n, cfg, (uint64_t *)us.p,
                       (uint64_t *)ue0.p, (uint32_t *)mpos.p, (uint32_t *)mread0.p, (uint32_t *)mnum0.p);
    size_t tb = 0;
    if (n_uni) {
      const unsigned bits = 32 + job.rid_bits;
      CM_HIPCHECK(c, rocprim::radix_sort_keys(nullptr, tb, (uint64_t *)ue0.p, (uint64_t *)ue1.p, (size_t)n_uni, 0, bits, s));
      if (tmp.ensure(tb + 256)) return job.enomem("allocation sort");
      CM_HIPCHECK(c, rocprim::radix_sort_keys(tmp.p, tb, (uint64_t *)ue0.p, (uint64_t *)ue1.p, (size_t)n_uni, 0, bits, s));
    }
    CM_HIPCHECK(c, rocprim::radix_sort_pairs(nullptr, tb, (uint32_t *)mread0.p, (uint32_t *)mread1.p, (uint32_t *)mnum0.p, (uint32_t *)mnum1.p,
                                             (size_t)n_multi, 0, 32, s));
    if (tmp.ensure(tb + 256)) return job.enomem("allocation sort");
    CM_HIPCHECK(c, rocprim::radix_sort_pairs(tmp.p, tb, (uint32_t *)mread0.p, (uint32_t *)mread1.p, (uint32_t *)mnum0.p, (uint32_t *)mnum1.p,
                                             (size_t)n_multi, 0, 32, s));
    const uint32_t *group_read = (const uint32_t *)mread1.p, *group_num = (const uint32_t *)mnum1.p;
    hipLaunchKernelGGL(k_al_weight, gm, b, 0, s, store, win, cfg, (const uint64_t *)us.p, (const uint64_t *)ue1.p, n_uni, (const uint32_t *)mpos.p,
                       group_read, group_num, n_multi, (int)p->multi_mapping_allocation_distance, (uint32_t *)wt.p, (uint32_t *)wh.p);
    CM_HIPCHECK(c, rocprim::inclusive_scan_by_key(nullptr, tb, group_read, (const uint32_t *)wt.p, (uint32_t *)sum.p, (size_t)n_multi,
                                                  rocprim::plus<uint32_t>(), rocprim::equal_to<uint32_t>(), s));
    if (tmp.ensure(tb + 256)) return job.enomem("allocation scan");
    CM_HIPCHECK(c, rocprim::inclusive_scan_by_key(tmp.p, tb, group_read, (const uint32_t *)wt.p, (uint32_t *)sum.p, (size_t)n_multi,
                                                  rocprim::plus<uint32_t>(), rocprim::equal_to<uint32_t>(), s));
    hipLaunchKernelGGL(k_al_count, gm, b, 0, s, group_read, (const uint32_t *)sum.p, n_multi, (unsigned long long *)cnt.p);
    // ---- the draw: one generator for the run, on the host
    std::vector<uint32_t> w(n_multi), kept;
    uint64_t counts[2] = {0, 0};
    CM_HIPCHECK(c, hipMemcpyAsync(counts, cnt.p, 16, hipMemcpyDeviceToHost, s));
    CM_HIPCHECK(c, hipMemcpyAsync(w.data(), wh.p, mb, hipMemcpyDeviceToHost, s));
    CM_HIPCHECK(c, cm_stream_sync(s));
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t without = cm_alloc_draw(w.data(), n_multi, p->multi_mapping_allocation_seed, kept);
    c->alloc_draw_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (kept.size() != counts[0] || without != counts[1]) { cm_set_error(c, "allocation: the device's group counts and the draw's disagree"); return CMGPU_EHIP; }
    c->alloc_kept = counts[0];
    c->alloc_without_overlap = counts[1];
    if (!kept.empty()) {
      if (kept_d.ensure(kept.size() * 4)) return job.enomem("allocation");
      CM_HIPCHECK(c, hipMemcpyAsync(kept_d.p, kept.data(), kept.size() * 4, hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_al_mark, dim3((unsigned)((kept.size() + PP_BLOCK - 1) / PP_BLOCK)), b, 0, s, (const uint32_t *)kept_d.p, (uint32_t)kept.size(),
                         group_num, (const uint32_t *)mpos.p, n_multi, n, (uint8_t *)keep.p);
    }
    hipLaunchKernelGGL(k_al_apply, g, b, 0, s, store, win, (const uint8_t *)keep.p, n, cfg, (uint64_t *)job.llen.p);
    CM_HIPCHECK(c, cm_stream_sync(s));  // (kept, and the buffers of this scope, are in use until here)
    return CMGPU_OK;
  }
  hipLaunchKernelGGL(k_al_apply, g, b, 0, s, store, win, (const uint8_t *)keep.p, n, cfg, (uint64_t *)job.llen.p);
  CM_HIPCHECK(c, cm_stream_sync(s));
  return CMGPU_OK;
}

extern "C" int cmgpu_store_allocation_info(const cmgpu_ctx *c, uint64_t *n_multi, uint64_t *n_allocated, uint64_t *n_without_overlap) {
  if (!c) return CMGPU_EINVAL;
  if (n_multi) *n_multi = c->alloc_multi;
  if (n_allocated) *n_allocated = c->alloc_kept;
  if (n_without_overlap) *n_without_overlap = c->alloc_without_overlap;
  return CMGPU_OK;
}

// ---------------------------------------------------------------------------------------
// sort + select + format
// ---------------------------------------------------------------------------------------
extern "C" int cmgpu_store_format(cmgpu_ctx *c, int kind, const char *const *names, uint32_t n_sequences, const cmgpu_params *p,
                                  uint32_t barcode_length, uint64_t *n_lines, uint64_t *n_bytes) {
  if (!c || !names || !p || !n_lines || !n_bytes) return CMGPU_EINVAL;
  if (kind < CMGPU_TEXT_BED_PE || kind > CMGPU_TEXT_TAGALIGN_SE_BC) { cm_set_error(c, "unknown text kind"); return CMGPU_EINVAL; }
  if (pp_has_bc(kind) != c->store_has_bc && c->store_n) { cm_set_error(c, "text kind does not match the stored records"); return CMGPU_EINVAL; }
  if (pp_has_bc(kind) && (barcode_length == 0 || barcode_length > 32)) { cm_set_error(c, "barcode length must be 1..32"); return CMGPU_EINVAL; }
  CM_HIPCHECK(c, cm_enter(c));
  { const int qrc = cm_exchange_quiesce(c); if (qrc) return qrc; }
  hipStream_t s = c->stream;
  *n_lines = 0;
  *n_bytes = 0;
  c->text_bytes = 0;
  c->text_lines = 0;
  c->alloc_multi = c->alloc_kept = c->alloc_without_overlap = 0;
  c->alloc_seconds = c->alloc_draw_seconds = 0;
  const uint32_t n = (uint32_t)c->store_n;
  if (n == 0) return CMGPU_OK;
  PpCfg cfg;
  cfg.kind = kind;
  cfg.dedup = p->remove_pcr_duplicates != 0;
  cfg.inmem = p->low_memory_mode == 0;
  cfg.tn5 = p->tn5_shift != 0;
  cfg.mapq_thr = p->mapq_threshold;
  cfg.n_seq = n_sequences;
  cfg.bc_len = barcode_length;
  cfg.bulk = pp_has_bc(kind) && p->dedup_at_bulk_level && p->low_memory_mode && p->remove_pcr_duplicates;
  cfg.last_section = 1;
  if (c->ex.transport)  // the merge loop's end-of-output rule (mapping_writer.h:331-337) belongs to the last rank that owns records
    for (int r = c->ex.rank + 1; r < c->ex.world; ++r) if (c->ex.owned_by[r]) cfg.last_section = 0;
  cfg.wl = (const uint64_t *)c->wl.p;
  cfg.wl_mask = c->wl_mask;
  // the translation table belongs to the kinds that print a barcode; every other kind runs as without one
  const bool translate = c->bt_entries != 0 && pp_prints_bc(kind);
  cfg.bt = translate ? cm_bt_dev(c) : CmBtDev{nullptr, nullptr, 0, 0};
  cfg.bt_miss = nullptr;
  // the reference allocates in its in-memory flavour only (chromap.h:1305-1353); with low_memory_mode the flag does nothing
  cfg.alloc = p->allocate_multi_mappings && !p->low_memory_mode;
  if (cfg.alloc && c->ex.transport) { cm_set_error(c, "allocate_multi_mappings: a read's positions lie on chromosomes of several ranks"); return CMGPU_EINVAL; }
  if (cfg.bulk && c->wl_size == 0) { cm_set_error(c, "bulk-level duplicate removal needs the whitelist abundances (cmgpu_set_whitelist)"); return CMGPU_EINVAL; }
  CmTextJob job;
  int rc;
  if ((rc = job.begin(c, names, n_sequences, n, 1, false))) return rc;
  const dim3 g((n + PP_BLOCK - 1) / PP_BLOCK), b(PP_BLOCK);
  const uint8_t *store = (const uint8_t *)c->store.p;
  const uint64_t *bc = (const uint64_t *)c->store_bc.p;
  hipLaunchKernelGGL(k_pp_key0, g, b, 0, s, store, n, job.keys(), job.idx());
  if ((rc = job.sort_pass(40))) return rc;
  if (pp_has_bc(kind)) {
    hipLaunchKernelGGL(k_pp_key_bc, g, b, 0, s, bc, (const uint32_t *)job.idx(), n, job.keys());
    if ((rc = job.sort_pass(2 * barcode_length))) return rc;
  }
  hipLaunchKernelGGL(k_pp_key_top, g, b, 0, s, store, (const uint32_t *)job.idx(), n, cfg, 0, job.keys());
  if ((rc = job.sort_pass(48 + (job.rid_bits > 16 ? 16 : job.rid_bits)))) return rc;
  if (job.rid_bits > 16) {
    hipLaunchKernelGGL(k_pp_key_top, g, b, 0, s, store, (const uint32_t *)job.idx(), n, cfg, 1, job.keys());
    if ((rc = job.sort_pass(job.rid_bits - 16))) return rc;
  }
  CM_HIPCHECK(c, cm_stream_sync(s));
  job.release_sort();
  // ---- select
  CmTmpBuf win, dups, longs;
  if (win.ensure((size_t)n * 4) || dups.ensure((size_t)n * 4)) return job.enomem("post-processing");
  if ((rc = job.alloc_lengths())) return rc;
  // heads of long duplicate runs: at most n / PP_RUN_SERIAL of them, + the counter
  if (longs.ensure(((size_t)n / PP_RUN_SERIAL + 2) * 4)) return job.enomem("post-processing");
  uint32_t *long_cnt = (uint32_t *)longs.p, *long_list = long_cnt + 1;
  if (hipMemsetAsync(long_cnt, 0, 4, s) != hipSuccess) { cm_set_error(c, "memset failed"); return CMGPU_EHIP; }
  // --barcode-translate: the selection counts the printed lines whose barcode the table lacks in the job's spare count word
  if (translate) {
    if ((rc = job.zero_counts())) return rc;
    cfg.bt_miss = job.extra_word();
  }
  // --summary: the selection credits every run to its survivor's barcode.  The keys are in the table since their reads were counted;
  // a store filled by the multi-GPU exchange also holds records of reads another context counted
  CmSmDev sm;
  if ((rc = cm_summary_dev(c, c->ex.transport ? n : 0, pp_has_bc(kind) && c->wl_size && !p->output_mappings_not_in_whitelist ? c->wl_size : 0,
                           !pp_has_bc(kind), &sm))) return rc;
  if (cfg.alloc && sm.keys) { cm_set_error(c, "allocate_multi_mappings: the summary's duplicate and low-MAPQ counts are taken before the allocation"); return CMGPU_EINVAL; }
  hipLaunchKernelGGL(k_pp_select, g, b, 0, s, store, bc, (const uint32_t *)job.idx(), n, cfg, job.seq_off(), (uint32_t *)win.p,
                     (uint32_t *)dups.p, (uint64_t *)job.llen.p, long_list, long_cnt, sm);
  hipLaunchKernelGGL(k_pp_select_long, dim3(1024), dim3(64), 0, s, store, bc, (const uint32_t *)job.idx(), n, cfg, job.seq_off(),
                     (uint32_t *)win.p, (uint32_t *)dups.p, (uint64_t *)job.llen.p, (const uint32_t *)long_list, (const uint32_t *)long_cnt, sm);
  if (cfg.alloc) {
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = pp_allocate(c, job, cfg, p, store, (const uint32_t *)win.p, n))) return rc;
    c->alloc_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();  // (pp_allocate ends with the stream waited for)
  }
  uint64_t total = 0, lines = 0, misses = 0;
  if ((rc = job.scan_lines(&total, &lines, translate ? &misses : nullptr))) return rc;
  if (misses) { cm_set_error(c, CM_BT_MISS_MESSAGE); return CMGPU_EFORMAT; }  // (no text: text_bytes is 0 since the call began)
  if ((rc = job.alloc_text(total))) return rc;
  // ---- format
  hipLaunchKernelGGL(k_pp_format, g, b, 0, s, store, bc, (const uint32_t *)win.p, (const uint32_t *)dups.p, (const uint64_t *)job.llen.p,
                     (const uint64_t *)job.loff.p, n, cfg, (const uint8_t *)job.names.p, job.seq_off(), (uint8_t *)c->text.p);
  return job.publish(total, lines, n_lines, n_bytes);
}

// ---------------------------------------------------------------------------------------
// pairs text (--preset hic) on the device: the store holds cmgpu_pairs_record entries, sorted by
// (rid1, rid2, pos1, pos2, mapq, read_id) as cmgpu_write_pairs / MappingWriter<PairsMapping> do (pairs_mapping.h:41-47),
// one line per record that passes the MAPQ filter: readID chrom1 pos1 chrom2 pos2 strand1 strand2 UU mapq mapq
// (mapping_writer.cc:400-423).  Read names: a blob + offsets indexed by read_id - read_id_base.  The "## pairs" header lines
// stay with the caller (cmgpu_pairs_header_text).
// ---------------------------------------------------------------------------------------
struct PpPairs { uint32_t read_id, rid1, rid2, pos1, pos2; uint8_t st1, st2, mapq, uniq; };
__device__ __forceinline__ PpPairs pp_load_pairs(const uint8_t *store, uint32_t i) {
  const uint64_t *p = reinterpret_cast<const uint64_t *>(store + (uint64_t)i * 24);
  const uint64_t a = p[0], b = p[1], c = p[2];
  PpPairs r;
  r.read_id = (uint32_t)a; r.rid1 = (uint32_t)(a >> 32); r.rid2 = (uint32_t)b; r.pos1 = (uint32_t)(b >> 32); r.pos2 = (uint32_t)c;
  r.st1 = (uint8_t)(c >> 32); r.st2 = (uint8_t)(c >> 40); r.mapq = (uint8_t)(c >> 48); r.uniq = (uint8_t)(c >> 56);
  return r;
}
// which: 0 = (mapq, read_id), 1 = (pos1, pos2), 2 = (rid1, rid2) with rid_bits each
__global__ __launch_bounds__(PP_BLOCK) void k_pp_pairs_key(const uint8_t *__restrict__ store, const uint32_t *__restrict__ idx, uint32_t n, int which,
                                                             unsigned rid_bits, uint64_t *__restrict__ key, uint32_t *__restrict__ idx_out) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = idx ? idx[j] : j;
  const PpPairs r = pp_load_pairs(store, i);
  key[j] = which == 0 ? ((uint64_t)r.mapq << 32) | r.read_id : which == 1 ? ((uint64_t)r.pos1 << 32) | r.pos2 : ((uint64_t)r.rid1 << rid_bits) | r.rid2;
  if (idx_out) idx_out[j] = i;
}
__global__ __launch_bounds__(PP_BLOCK) void k_pp_pairs_len(const uint8_t *__restrict__ store, const uint32_t *__restrict__ idx, uint32_t n, int mapq_thr,
                                                             uint32_t n_seq, const uint32_t *__restrict__ name_off, const uint64_t *__restrict__ rn_off,
                                                             uint32_t rn_base, uint32_t rn_count, uint64_t *__restrict__ line_len, int dedup, CmSmDev sm) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const PpPairs r = pp_load_pairs(store, idx[j]);
  const uint32_t q = r.read_id - rn_base;
  if (sm.keys && r.rid1 < n_seq && r.rid2 < n_seq && q < rn_count) {
    // --summary: the first record of a run (every record without duplicate removal) counts the run; its last record has the run's largest
    // MAPQ, which is the survivor's under either rule.  A PairsMapping has no barcode (GetBarcode() == 0): everything counts under key 0
    auto same_run = [&](const PpPairs &x) { return x.rid1 == r.rid1 && x.pos1 == r.pos1 && x.rid2 == r.rid2 && x.pos2 == r.pos2; };
    if (!dedup || j == 0 || !same_run(pp_load_pairs(store, idx[j - 1]))) {
      uint32_t d = 1, mq = r.mapq;
      for (uint32_t t = j + 1; dedup && t < n; ++t, ++d) {
        const PpPairs nx = pp_load_pairs(store, idx[t]);
        if (!same_run(nx)) break;
        mq = nx.mapq;
      }
      if (dedup == 2 && d > 255) d = 255;
      cm_sm_credit(sm, true, 0, d, (int)mq >= mapq_thr);
    }
  }
  if ((int)r.mapq < mapq_thr || r.rid1 >= n_seq || r.rid2 >= n_seq || q >= rn_count) { line_len[j] = 0; return; }
  // --remove-pcr-duplicates: one record per run of PairsMapping::operator== (rid1, pos1, rid2, pos2; pairs_mapping.h:45-50).  The records
  // stand in operator< order, i.e. inside a run by (mapq, read_id).  dedup == 1, the low-memory merge (mapping_writer.h:244-270): the
  // FIRST record with the run's largest MAPQ (a later one replaces the survivor only when its MAPQ is larger); dedup == 2, the
  // in-memory RemovePCRDuplicate (mapping_processor.h:178-195): the LAST of the run.  The MAPQ filter above is the survivor's:
  // the run's largest MAPQ either way, so a record below the threshold is never a survivor that would have passed.
  if (dedup) {
    auto same_key = [&](const PpPairs &x) { return x.rid1 == r.rid1 && x.pos1 == r.pos1 && x.rid2 == r.rid2 && x.pos2 == r.pos2; };
    bool win;
    if (dedup == 2) {
      win = j + 1 == n || !same_key(pp_load_pairs(store, idx[j + 1]));
    } else {
      win = j == 0;
      if (!win) { const PpPairs pr = pp_load_pairs(store, idx[j - 1]); win = !same_key(pr) || pr.mapq != r.mapq; }  // first of its (run, MAPQ) group ...
      for (uint32_t t = j + 1; win && t < n; ++t) {                                                               // ... and no larger MAPQ follows in the run
        const PpPairs nx = pp_load_pairs(store, idx[t]);
        if (!same_key(nx)) break;
        if (nx.mapq != r.mapq) win = false;
      }
    }
    if (!win) { line_len[j] = 0; return; }
  }
  const uint32_t rn = (uint32_t)(rn_off[q + 1] - rn_off[q]);
  line_len[j] = rn + 1 + (name_off[r.rid1 + 1] - name_off[r.rid1]) + 1 + cm_digits10(r.pos1 + 1) + 1 + (name_off[r.rid2 + 1] - name_off[r.rid2]) + 1 +
                cm_digits10(r.pos2 + 1) + 2 + 2 + 4 + cm_digits10(r.mapq) + 1 + cm_digits10(r.mapq) + 1;
}
__global__ __launch_bounds__(PP_BLOCK) void k_pp_pairs_format(const uint8_t *__restrict__ store, const uint32_t *__restrict__ idx, uint32_t n,
                                                                const uint64_t *__restrict__ line_len, const uint64_t *__restrict__ line_off,
                                                                const uint8_t *__restrict__ names, const uint32_t *__restrict__ name_off,
                                                                const uint8_t *__restrict__ rn, const uint64_t *__restrict__ rn_off, uint32_t rn_base,
                                                                uint8_t *__restrict__ text) {
  const uint32_t j = blockIdx.x * PP_BLOCK + threadIdx.x;
  if (j >= n || line_len[j] == 0) return;
  const PpPairs r = pp_load_pairs(store, idx[j]);
  uint8_t *p = text + line_off[j];
  const uint32_t q = r.read_id - rn_base;
  for (uint64_t i = rn_off[q]; i < rn_off[q + 1]; ++i) *p++ = rn[i];
  *p++ = '\t';
  for (uint32_t i = name_off[r.rid1]; i < name_off[r.rid1 + 1]; ++i) *p++ = names[i];
  *p++ = '\t';
  p = cm_put_u32(p, r.pos1 + 1);
  *p++ = '\t';
  for (uint32_t i = name_off[r.rid2]; i < name_off[r.rid2 + 1]; ++i) *p++ = names[i];
  *p++ = '\t';
  p = cm_put_u32(p, r.pos2 + 1);
  *p++ = '\t'; *p++ = r.st1 ? '+' : '-';
  *p++ = '\t'; *p++ = r.st2 ? '+' : '-';
  *p++ = '\t'; *p++ = 'U'; *p++ = 'U'; *p++ = '\t';
  p = cm_put_u32(p, r.mapq);
  *p++ = '\t';
  p = cm_put_u32(p, r.mapq);
  *p++ = '\n';
}

// the body of cmgpu_store_format_pairs and cmgpu_store_format_pairs_resident.  resident: the read names are the context's name store
// (cm_ingest.hip), read by the kernels above where they lie; otherwise the caller's host blob and offsets are uploaded first.
static int pp_format_pairs(cmgpu_ctx *c, const char *const *names, uint32_t n_sequences, const cmgpu_params *p, bool resident,
                           const char *read_names, const uint64_t *read_name_offsets, uint32_t n_read_names,
                           uint32_t read_id_base, uint64_t *n_lines, uint64_t *n_bytes) {
  if (p->allocate_multi_mappings && !p->low_memory_mode) { cm_set_error(c, "allocate_multi_mappings: pairs records have no allocation stage"); return CMGPU_EINVAL; }
  if (!cm_store_pairs_records(c)) { cm_set_error(c, "pairs text needs pairs records (split alignment, or output_format = CMGPU_FORMAT_PAIRS)"); return CMGPU_EINVAL; }
  // (cell barcodes: they decided which pairs were mapped -- CorrectBarcodeAt, chromap.h:896-906 -- and go no further: a PairsMapping's barcode is
  //  neither printed nor part of its order or equality, pairs_mapping.h:40-50, GetBarcode() == 0; the store's key array is left alone)
  CM_HIPCHECK(c, cm_enter(c));
  { const int qrc = cm_exchange_quiesce(c); if (qrc) return qrc; }
  hipStream_t s = c->stream;
  *n_lines = 0;
  *n_bytes = 0;
  c->text_bytes = 0;
  c->text_lines = 0;
  const uint32_t n = (uint32_t)c->store_n;
  if (n == 0) return CMGPU_OK;
  const uint64_t rn_bytes = !resident && n_read_names ? read_name_offsets[n_read_names] : 0;
  CmTextJob job;
  CmTmpBuf d_rn, d_rnoff;  // (allocated before the job uploads anything)
  if (d_rn.ensure(rn_bytes + 16) || d_rnoff.ensure(resident ? 8 : ((size_t)n_read_names + 1) * 8)) { cm_set_error(c, "out of device memory (post-processing)"); return CMGPU_ENOMEM; }
  int rc;
  if ((rc = job.begin(c, names, n_sequences, n, 1, true))) return rc;
  const uint64_t zero = 0;
  if ((rn_bytes && hipMemcpyAsync(d_rn.p, read_names, rn_bytes, hipMemcpyHostToDevice, s) != hipSuccess) ||
      hipMemcpyAsync(d_rnoff.p, !resident && n_read_names ? (const void *)read_name_offsets : (const void *)&zero,
                     resident ? 8 : ((size_t)n_read_names + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess) {
    cm_set_error(c, "name upload failed"); return CMGPU_EHIP;
  }
  // (no names at all: the one zero offset uploaded above stands for an empty table)
  const uint8_t *rn = resident && n_read_names ? (const uint8_t *)c->nm_blob.p : (const uint8_t *)d_rn.p;
  const uint64_t *rn_off = resident && n_read_names ? (const uint64_t *)c->nm_offs.p : (const uint64_t *)d_rnoff.p;
  const dim3 g((n + PP_BLOCK - 1) / PP_BLOCK), b(PP_BLOCK);
  const uint8_t *store = (const uint8_t *)c->store.p;
  const unsigned rid_bits = job.rid_bits;
  // least significant key first: (mapq, read_id), then (pos1, pos2), then (rid1, rid2) -- stable radix passes
  hipLaunchKernelGGL(k_pp_pairs_key, g, b, 0, s, store, (const uint32_t *)nullptr, n, 0, rid_bits, job.keys(), job.idx());
  if ((rc = job.sort_pass(40))) return rc;
  hipLaunchKernelGGL(k_pp_pairs_key, g, b, 0, s, store, (const uint32_t *)job.idx(), n, 1, rid_bits, job.keys(), (uint32_t *)nullptr);
  if ((rc = job.sort_pass(64))) return rc;
  hipLaunchKernelGGL(k_pp_pairs_key, g, b, 0, s, store, (const uint32_t *)job.idx(), n, 2, rid_bits, job.keys(), (uint32_t *)nullptr);
  if ((rc = job.sort_pass(2 * rid_bits))) return rc;
  CmSmDev sm;
  if ((rc = cm_summary_dev(c, 0, 0, true, &sm))) return rc;
  hipLaunchKernelGGL(k_pp_pairs_len, g, b, 0, s, store, (const uint32_t *)job.idx(), n, p->mapq_threshold, n_sequences, job.seq_off(),
                     rn_off, read_id_base, n_read_names, (uint64_t *)job.llen.p,
                     p->remove_pcr_duplicates ? (p->low_memory_mode ? 1 : 2) : 0, sm);
  uint64_t total = 0, lines = 0;
  if ((rc = job.scan_lines(&total, &lines))) return rc;
  if ((rc = job.alloc_text(total))) return rc;
  hipLaunchKernelGGL(k_pp_pairs_format, g, b, 0, s, store, (const uint32_t *)job.idx(), n, (const uint64_t *)job.llen.p, (const uint64_t *)job.loff.p,
                     (const uint8_t *)job.names.p, job.seq_off(), rn, rn_off, read_id_base, (uint8_t *)c->text.p);
  return job.publish(total, lines, n_lines, n_bytes);
}

extern "C" int cmgpu_store_format_pairs(cmgpu_ctx *c, const char *const *names, uint32_t n_sequences, const cmgpu_params *p,
                                        const char *read_names, const uint64_t *read_name_offsets, uint32_t n_read_names,
                                        uint32_t read_id_base, uint64_t *n_lines, uint64_t *n_bytes) {
  if (!c || !names || !p || !n_lines || !n_bytes || (!read_names && n_read_names) || (!read_name_offsets && n_read_names)) return CMGPU_EINVAL;
  return pp_format_pairs(c, names, n_sequences, p, false, read_names, read_name_offsets, n_read_names, read_id_base, n_lines, n_bytes);
}
// the same with the read names the device ingest kept (cmgpu_fastq_keep_names): nothing is uploaded or copied
extern "C" int cmgpu_store_format_pairs_resident(cmgpu_ctx *c, const char *const *names, uint32_t n_sequences, const cmgpu_params *p,
                                                 uint64_t *n_lines, uint64_t *n_bytes) {
  if (!c || !names || !p || !n_lines || !n_bytes) return CMGPU_EINVAL;
  if (c->nm_n > 0xffffffffull) { cm_set_error(c, "more than 2^32 read names"); return CMGPU_ECAPACITY; }
  return pp_format_pairs(c, names, n_sequences, p, true, nullptr, nullptr, (uint32_t)c->nm_n, c->nm_base, n_lines, n_bytes);
}

extern "C" int cmgpu_store_text(cmgpu_ctx *c, char *out, uint64_t capacity) {
  if (!c || (!out && c->text_bytes)) return CMGPU_EINVAL;
  if (capacity < c->text_bytes) { cm_set_error(c, "text buffer too small"); return CMGPU_ECAPACITY; }
  CM_HIPCHECK(c, cm_enter(c));
  if (c->text_bytes) CM_HIPCHECK(c, hipMemcpy(out, c->text.p, c->text_bytes, hipMemcpyDeviceToHost));
  return CMGPU_OK;
}

// (round 6: this took 89 ms for 246 MB where a bare write() of as many bytes takes 25 -- a 64 MiB page-locked slab costs ~35 ms to allocate
//  and more to free, and copies and writes took turns.  Now two ordinary 16 MiB slabs: the runtime's own staging buffers bring a copy into
//  pageable memory at ~25 GB/s, and a second thread writes one slab while the next is being copied.  Several writing threads gain nothing:
//  buffered writes to one file are serialised by the kernel -- tools/probes/write_probe.cpp, 1 / 4 / 16 threads 25 / 25 / 32 ms per 256 MB)
int cm_write_device_bytes(cmgpu_ctx *c, const void *dev, uint64_t n_bytes, const char *path, int append, const char *what) {
  FILE *f = fopen(path, append ? "ab" : "wb");
  if (!f) { cm_set_error(c, std::string("cannot open ") + path); return CMGPU_EIO; }
  const size_t slab = 16u << 20;
  const uint64_t n_slabs = (n_bytes + slab - 1) / slab;
  std::vector<uint8_t> buf[2];
  for (int k = 0; k < 2 && (uint64_t)k < n_slabs; ++k) buf[k].resize(n_slabs == 1 ? (size_t)n_bytes : slab);
  // slab i is copied into buf[i & 1] once slab i - 2 has been written out of it
  std::mutex mu;
  std::condition_variable cv;
  uint64_t copied = 0, written = 0;  // slabs copied / written so far
  bool ok = true;
  std::thread writer([&]() {
    for (uint64_t i = 0; i < n_slabs; ++i) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&]() { return copied > i || !ok; });
        if (!ok) return;
      }
      const uint64_t o = i * slab;
      const size_t m = n_bytes - o < slab ? (size_t)(n_bytes - o) : slab;
      const bool w = fwrite(buf[i & 1].data(), 1, m, f) == m;
      std::lock_guard<std::mutex> lk(mu);
      if (!w) ok = false;
      written = i + 1;
      cv.notify_all();
      if (!w) return;
    }
  });
  bool copy_failed = false;
  for (uint64_t i = 0; i < n_slabs; ++i) {
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&]() { return i < 2 || written + 2 > i || !ok; });
      if (!ok) break;
    }
    const uint64_t o = i * slab;
    const size_t m = n_bytes - o < slab ? (size_t)(n_bytes - o) : slab;
    const bool cp = hipMemcpy(buf[i & 1].data(), (const uint8_t *)dev + o, m, hipMemcpyDeviceToHost) == hipSuccess;
    std::lock_guard<std::mutex> lk(mu);
    if (!cp) { ok = false; copy_failed = true; }
    else copied = i + 1;
    cv.notify_all();
    if (!cp) break;
  }
  writer.join();
  ok = fclose(f) == 0 && ok;
  if (copy_failed) { (void)hipGetLastError(); cm_set_error(c, std::string("copying ") + what + " from the device failed"); return CMGPU_EHIP; }
  if (!ok) { cm_set_error(c, std::string("short write to ") + path); return CMGPU_EIO; }
  return CMGPU_OK;
}
extern "C" int cmgpu_store_write_text(cmgpu_ctx *c, const char *path, int append) {
  if (!c || !path) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  return cm_write_device_bytes(c, c->text.p, c->text_bytes, path, append, "the rendered text");
}

extern "C" int cmgpu_store_info(const cmgpu_ctx *c, uint64_t *n_records, uint64_t *text_bytes, uint64_t *text_lines) {
  if (!c) return CMGPU_EINVAL;
  if (n_records) *n_records = c->store_n;
  if (text_bytes) *text_bytes = c->text_bytes;
  if (text_lines) *text_lines = c->text_lines;
  return CMGPU_OK;
}

// n 32-byte {record, barcode} entries (the receive side of the multi-GPU exchange, cm_exchange.hip) -> the store's
// record and barcode arrays at position store_n; the caller advances store_n
void cm_store_split_bc(cmgpu_ctx *c, const void *in32, uint64_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_pp_split_bc, dim3((unsigned)((n + PP_BLOCK - 1) / PP_BLOCK)), dim3(PP_BLOCK), 0, s, (const uint8_t *)in32, (uint32_t)n,
                     (uint8_t *)c->store.p + c->store_n * 24, (uint64_t *)c->store_bc.p + c->store_n);
}

int cm_compact_records(cmgpu_ctx *c, void *dst, uint64_t *bc_dst, uint64_t cap, hipStream_t s, const uint32_t **n_valid_dev) {
  const uint32_t n = (uint32_t)cm_rec_slots(c);
  { const int rc = cm_ensure_slot_scratch(c, n); if (rc) return rc; }
  uint32_t *flag = (uint32_t *)c->scratch_a.p, *pos = (uint32_t *)c->scratch_b.p;  // free between batches
  const dim3 g((n + PP_BLOCK - 1) / PP_BLOCK), b(PP_BLOCK);
  hipLaunchKernelGGL(k_pp_flag, g, b, 0, s, (const uint8_t *)c->rec_ok.p, flag, n);
  cm_scan_u32(flag, pos, n, (uint32_t *)c->scan_tmp.p, s);
  hipLaunchKernelGGL(k_pp_compact, g, b, 0, s, (const uint8_t *)c->rec.p, (const uint8_t *)c->rec_ok.p, (const uint32_t *)pos,
                     (const uint64_t *)c->bc_key.p, (uint8_t *)dst, bc_dst, n, cm_rec_per_pair(c), cap);
  if (n_valid_dev) *n_valid_dev = pos + n;
  return CMGPU_OK;
}

// the device code of this translation unit is loaded by the HIP runtime at the first launch of one of its kernels (milliseconds to tens of
// milliseconds for the larger ones): context creation launches this empty kernel so that a job's first batch does not pay for it (cm_api.hip: cm_load_device_code)
__global__ void k_touch_post() {}
void cm_touch_post(hipStream_t s) { hipLaunchKernelGGL(k_touch_post, dim3(1), dim3(1), 0, s); }
