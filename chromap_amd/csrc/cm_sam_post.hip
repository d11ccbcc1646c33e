// cm_sam_post.hip -- SAM output on the device: record store, sort, duplicate removal, MAPQ filter and text in HBM.
// Replaces, for runs that go through the device ingest, the host writer cmgpu_write_sam* (cm_host.cpp: write_sam_impl), i.e.
// MappingWriter<SAMMapping>::AppendMapping (mapping_writer.cc:312-356) behind the sort and duplicate handling of
// SAMMapping::operator< / operator== (sam_mapping.h:193-212).  The bytes are the host writer's.
//
//   store:  after every cmgpu_map_resident the batch's VALID slots (record, CIGAR words, MD bytes, the pair's barcode key) are
//           compacted behind the run's -- the fixed 64-word / md_cap slots of the batch pools are mostly empty and stay per batch
//   format: stable least-significant-first radix passes over an index array for (rid, pos, barcode, mrid, mpos, flag & 64, mapq,
//           read_id); a length kernel (duplicate rule, filter, line length), a 64-bit scan, and the format kernel: a GROUP of lanes
//           per line -- one lane writes the short numeric fields, the group copies name, SEQ, QUAL and MD from the read store
//           (cm_ingest.hip) with word-wide stores where the destination is aligned
//   BAM:    cmgpu_store_format_bam runs the same passes and the same length kernel; a selected record's length is that of its BAM
//           alignment record and the format kernel writes that record (cm_bam.h) where k_sp_format writes the line
#include <hip/hip_runtime.h>
#include <string.h>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include <cstdio>
#include <string>
#include <vector>

#include "cm_bam.h"
#include "cm_ctx.h"
#include "cm_kernels.h"
#include "cm_summary.h"
#include "cm_text_job.h"

#define SP_BLOCK 256

struct SpRec {  // cmgpu_sam_record (40 bytes, include/chromap_amd.h), read with five 8-byte loads
  uint32_t read_id, rid, pos, mpos, nm;
  int32_t mrid, tlen;
  uint32_t flag, n_cigar, md_len, mapq, strand, valid, trim_len;
};
__device__ __forceinline__ SpRec sp_load(const uint8_t *rec, uint64_t i) {
  const uint64_t *p = reinterpret_cast<const uint64_t *>(rec + i * 40);
  const uint64_t a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
  SpRec r;
  r.read_id = (uint32_t)a; r.rid = (uint32_t)(a >> 32); r.pos = (uint32_t)b; r.mpos = (uint32_t)(b >> 32);
  r.mrid = (int32_t)(uint32_t)c; r.tlen = (int32_t)(uint32_t)(c >> 32);
  r.nm = (uint32_t)d; r.flag = (uint32_t)(d >> 32) & 0xffffu; r.n_cigar = (uint32_t)(d >> 48);
  r.md_len = (uint32_t)e & 0xffffu; r.mapq = (uint32_t)(e >> 16) & 0xffu; r.strand = (uint32_t)(e >> 24) & 0xffu;
  r.valid = (uint32_t)(e >> 40) & 0xffu; r.trim_len = (uint32_t)(e >> 48);
  return r;
}
__device__ __forceinline__ uint32_t sp_var_bytes(uint32_t n_cigar, uint32_t md_len) { return 4u * n_cigar + ((md_len + 3u) & ~3u); }

// ---------------------------------------------------------------------------------------
// record store
// ---------------------------------------------------------------------------------------
// per slot of the batch: kept or not, and the bytes of its variable part; a slot whose alignment did not fit the CIGAR slot (valid == 2) is reported
__global__ __launch_bounds__(SP_BLOCK) void k_sp_flag(const uint8_t *__restrict__ rec, uint32_t n, uint32_t *__restrict__ flag, uint64_t *__restrict__ vlen,
                                                        uint32_t *__restrict__ overflow) {
  const uint32_t i = blockIdx.x * SP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const SpRec r = sp_load(rec, i);
  if (r.valid == 2) atomicMin(overflow, i);
  flag[i] = r.valid == 1 ? 1u : 0u;
  vlen[i] = r.valid == 1 ? sp_var_bytes(r.n_cigar, r.md_len) : 0u;
}
// the kept slots behind the store's records: the record (its valid byte becomes 1 + mate), CIGAR words + MD bytes, the barcode key
__global__ __launch_bounds__(SP_BLOCK) void k_sp_compact(const uint8_t *__restrict__ rec, const uint32_t *__restrict__ cigar, const uint8_t *__restrict__ md,
                                                           uint32_t md_cap, const uint64_t *__restrict__ bc_key, const uint32_t *__restrict__ flag,
                                                           const uint32_t *__restrict__ pos, const uint64_t *__restrict__ voff, uint32_t n, int paired,
                                                           uint64_t var_base, uint8_t *__restrict__ out_rec, uint8_t *__restrict__ out_var,
                                                           uint64_t *__restrict__ out_voff, uint64_t *__restrict__ out_bc) {
  const uint32_t i = blockIdx.x * SP_BLOCK + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const uint32_t k = pos[i];
  const uint64_t *s = reinterpret_cast<const uint64_t *>(rec + (uint64_t)i * 40);
  uint64_t *d = reinterpret_cast<uint64_t *>(out_rec + (uint64_t)k * 40);
  const uint64_t mate = paired ? (i & 1u) : 0u, e = s[4];
  d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
  d[4] = (e & ~(0xffull << 40)) | ((1ull + mate) << 40);
  const uint32_t n_cigar = (uint32_t)(s[3] >> 48), md_len = (uint32_t)e & 0xffffu;
  const uint64_t vo = var_base + voff[i];
  out_voff[k + 1] = vo + sp_var_bytes(n_cigar, md_len);  // (entry 0 of the store's offsets is written once, by the host)
  uint32_t *w = reinterpret_cast<uint32_t *>(out_var + vo);
  const uint32_t *cg = cigar + (uint64_t)i * CM_SAM_CIGAR_CAP;
  for (uint32_t t = 0; t < n_cigar; ++t) w[t] = cg[t];
  w += n_cigar;
  const uint8_t *m = md + (uint64_t)i * md_cap;
  for (uint32_t t = 0; t < md_len; t += 4) {  // (the source slot has no alignment of its own: bytes in, words out)
    uint32_t x = 0;
    for (uint32_t b = 0; b < 4 && t + b < md_len; ++b) x |= (uint32_t)m[t + b] << (8 * b);
    w[t / 4] = x;
  }
  if (out_bc) out_bc[k] = bc_key[paired ? i / 2 : i];
}

extern "C" int cmgpu_sam_store_clear(cmgpu_ctx *c) {
  if (!c) return CMGPU_EINVAL;
  c->ss.n = 0;
  c->ss.var_bytes = 0;
  c->ss.has_bc = false;
  c->ss.paired = false;
  return CMGPU_OK;
}
extern "C" int cmgpu_sam_store_info(const cmgpu_ctx *c, uint64_t *n_records, uint64_t *n_bytes) {
  if (!c) return CMGPU_EINVAL;
  if (n_records) *n_records = c->ss.n;
  if (n_bytes) *n_bytes = c->ss.n * (40 + 8 + (c->ss.has_bc ? 8 : 0)) + c->ss.var_bytes;
  return CMGPU_OK;
}

extern "C" int cmgpu_sam_store_append_resident(cmgpu_ctx *c, uint64_t *n_total) {
  if (!c) return CMGPU_EINVAL;
  if (!c->p.sam) { cm_set_error(c, "the ctx was not created with output_format = CMGPU_FORMAT_SAM"); return CMGPU_EINVAL; }
  CM_HIPCHECK(c, cm_enter(c));
  CmSamStore &st = c->ss;
  const uint64_t slots = c->n_pairs ? c->sam_slots : 0;
  if (st.n && slots && (st.has_bc != c->has_barcodes || st.paired != !c->single)) {
    cm_set_error(c, "SAM record store mixes batches of different kinds (barcoded / bulk, paired / single-end)"); return CMGPU_EINVAL;
  }
  if (slots) {
    hipStream_t s = c->stream;
    const uint32_t n = (uint32_t)slots;
    int rc = cm_ensure_slot_scratch(c, n);
    if (rc) return rc;
    DevBuf &vlen = st.vlen, &voff = st.voff, &tmp = st.scan_tmp, &ovf = st.flags;  // (kept with the context: no allocation or free per batch)
    if (vlen.ensure(((size_t)n + 1) * 8) || voff.ensure(((size_t)n + 1) * 8) || ovf.ensure(4)) { cm_set_error(c, "out of device memory (SAM record store: scan)"); return CMGPU_ENOMEM; }
    uint32_t *flag = (uint32_t *)c->scratch_a.p, *pos = (uint32_t *)c->scratch_b.p;  // free between batches
    const dim3 g((n + SP_BLOCK - 1) / SP_BLOCK), b(SP_BLOCK);
    hipError_t e = hipMemsetAsync(ovf.p, 0xff, 4, s);
    if (e == hipSuccess) e = hipMemsetAsync((uint64_t *)vlen.p + n, 0, 8, s);
    if (e != hipSuccess) { cm_set_error(c, std::string("SAM record store: ") + hipGetErrorString(e)); return CMGPU_EHIP; }
    hipLaunchKernelGGL(k_sp_flag, g, b, 0, s, (const uint8_t *)c->sam_rec.p, n, flag, (uint64_t *)vlen.p, (uint32_t *)ovf.p);
    cm_scan_u32(flag, pos, n, (uint32_t *)c->scan_tmp.p, s);
    rc = cm_scan_u64(c, (const uint64_t *)vlen.p, (uint64_t *)voff.p, (size_t)n + 1, tmp, s, "SAM record store: scan");
    if (rc) return rc;
    uint32_t k = 0, over = 0;
    uint64_t vbytes = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&k, pos + n, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&vbytes, (uint64_t *)voff.p + n, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&over, ovf.p, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = cm_stream_sync(s);
    if (e != hipSuccess) { cm_set_error(c, std::string("SAM record store: ") + hipGetErrorString(e)); return CMGPU_EHIP; }
    if (over != 0xffffffffu) { cm_set_error(c, "an alignment needs more than CMGPU_SAM_CIGAR_CAP CIGAR operations"); return CMGPU_ECAPACITY; }
    if (st.n + k > 0xfffffff0ull) { cm_set_error(c, "SAM record store is limited to 2^32 records"); return CMGPU_ECAPACITY; }
    if (k) {
      const bool first = st.n == 0;
      rc = cm_grow_buf(c, st.rec, st.n * 40, (st.n + k) * 40 + 16, 64u << 20, s, "SAM record store: records");
      if (!rc) rc = cm_grow_buf(c, st.var_offs, first ? 0 : (st.n + 1) * 8, (st.n + k + 1) * 8, 16u << 20, s, "SAM record store: offsets");
      if (!rc) rc = cm_grow_buf(c, st.var, st.var_bytes, st.var_bytes + vbytes + 16, 64u << 20, s, "SAM record store: CIGAR and MD");
      if (!rc && c->has_barcodes) rc = cm_grow_buf(c, st.bc, st.n * 8, (st.n + k) * 8, 16u << 20, s, "SAM record store: barcodes");
      if (rc) return rc;
      if (first) {
        if ((e = hipMemsetAsync(st.var_offs.p, 0, 8, s)) != hipSuccess) { cm_set_error(c, std::string("SAM record store: ") + hipGetErrorString(e)); return CMGPU_EHIP; }
        st.has_bc = c->has_barcodes;
        st.paired = !c->single;
      }
      hipLaunchKernelGGL(k_sp_compact, g, b, 0, s, (const uint8_t *)c->sam_rec.p, (const uint32_t *)c->sam_cigar.p, (const uint8_t *)c->sam_md.p,
                         c->sam_md_cap, (const uint64_t *)c->bc_key.p, (const uint32_t *)flag, (const uint32_t *)pos, (const uint64_t *)voff.p, n,
                         c->single ? 0 : 1, st.var_bytes, (uint8_t *)st.rec.p + st.n * 40, (uint8_t *)st.var.p, (uint64_t *)st.var_offs.p + st.n,
                         c->has_barcodes ? (uint64_t *)st.bc.p + st.n : (uint64_t *)nullptr);
      e = cm_stream_sync(s);
      if (e != hipSuccess) { cm_set_error(c, std::string("SAM record store: ") + hipGetErrorString(e)); return CMGPU_EHIP; }
      st.n += k;
      st.var_bytes += vbytes;
    }
  }
  if (n_total) *n_total = st.n;
  return CMGPU_OK;
}

// ---------------------------------------------------------------------------------------
// sort + duplicates + filter + text
// ---------------------------------------------------------------------------------------
struct SpCfg {
  uint32_t n_seq, bc_len, base;   // sequences of the reference; barcode length (0: bulk); read id of the read store's first read
  uint64_t n_reads;               // reads per mate in the read store
  int mapq_thr, dedup;            // dedup: 0 off, 1 low-memory rule (first record of the run's largest MAPQ), 2 in-memory rule (last of the run)
  CmBtDev bt;                     // --barcode-translate: the CB:Z: value through the table (bt.tab == nullptr: Seed2Sequence)
};
struct SpReads {  // the read store, per mate (cm_ingest.hip)
  const uint8_t *names[2], *bases[2], *quals[2];
  const uint64_t *name_offs[2], *offs[2];
};
// which: 0 (mapq, read_id); 1 (mpos, flag & 64); 2 mrid + 1 (no mate, -1, first); 3 barcode; 4 (rid, pos)
__global__ __launch_bounds__(SP_BLOCK) void k_sp_key(const uint8_t *__restrict__ rec, const uint64_t *__restrict__ bc, const uint32_t *__restrict__ idx,
                                                       uint32_t n, int which, uint32_t n_seq, uint64_t *__restrict__ key, uint32_t *__restrict__ idx_out) {
  const uint32_t j = blockIdx.x * SP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = idx ? idx[j] : j;
  uint64_t k;
  if (which == 3) k = bc[i];
  else {
    const SpRec r = sp_load(rec, i);
    const uint32_t rid = r.rid < n_seq ? r.rid : n_seq;  // (a record of no sequence is never printed; it only has to sort somewhere)
    const uint32_t mr = r.mrid < 0 ? 0u : ((uint32_t)r.mrid < n_seq ? (uint32_t)r.mrid + 1u : n_seq + 1u);
    k = which == 0 ? ((uint64_t)r.mapq << 32) | r.read_id : which == 1 ? ((uint64_t)r.mpos << 1) | ((r.flag >> 6) & 1u) : which == 2 ? (uint64_t)mr
                                                                                                                            : ((uint64_t)rid << 32) | r.pos;
  }
  key[j] = k;
  if (idx_out) idx_out[j] = i;
}
__device__ __forceinline__ bool sp_same_run(const SpRec &x, uint64_t xb, const SpRec &y, uint64_t yb) {  // SAMMapping::operator== (sam_mapping.h:200-212)
  return x.pos == y.pos && x.rid == y.rid && xb == yb && (x.flag & 64u) == (y.flag & 64u) && x.mrid == y.mrid && x.mpos == y.mpos;
}
// bases of the read that are printed: the first length_after_trim, cut to the CIGAR's query length (SAMMapping::GetSequenceLength, sam_mapping.h:246-256);
// *cig_text: characters of the CIGAR column
__device__ __forceinline__ uint32_t sp_seq_len(const SpRec &r, const uint32_t *__restrict__ cg, uint32_t *cig_text) {
  uint32_t ql = 0, ct = 0;
  for (uint32_t t = 0; t < r.n_cigar; ++t) {
    const uint32_t w = cg[t], op = w & 0xfu;
    if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ql += w >> 4;
    ct += cm_digits10(w >> 4) + 1u;
  }
  *cig_text = r.n_cigar ? ct : 1u;
  return ql < r.trim_len ? ql : r.trim_len;
}
// BAM: the length is that of the BAM alignment record (cm_bam.h), and a printed record whose read name does not fit l_read_name counts
template <bool BAM>
__global__ __launch_bounds__(SP_BLOCK) void k_sp_len(const uint8_t *__restrict__ rec, const uint64_t *__restrict__ bc, const uint8_t *__restrict__ var,
                                                       const uint64_t *__restrict__ var_offs, const uint32_t *__restrict__ idx, uint32_t n, SpCfg cfg,
                                                       SpReads rs, const uint32_t *__restrict__ name_off, uint64_t *__restrict__ line_len,
                                                       unsigned long long *__restrict__ counts, CmSmDev sm) {
  // counts[0]: records that belong to no read of the read store; counts[1]: lines whose barcode the translation table does not have;
  // counts[2]: BAM records whose read name has more than CM_BAM_NAME_MAX bytes
  const uint32_t j = blockIdx.x * SP_BLOCK + threadIdx.x;
  if (j >= n) return;
  const uint32_t i = idx[j];
  const SpRec r = sp_load(rec, i);
  const uint64_t q = (uint64_t)(r.read_id - cfg.base);
  // a record whose read is not in the read store, or whose mate lies on a sequence the reference does not have: the stores are not of one
  // run -- counted, and the call fails (no line is written for it: the kernels never index past a store)
  if (q >= cfg.n_reads || (r.mrid >= 0 && (uint32_t)r.mrid >= cfg.n_seq)) { atomicAdd(counts, 1ull); line_len[j] = 0; return; }
  if (sm.keys && r.rid < cfg.n_seq) {
    // --summary (mapping_writer.h:281-301, 420-432): the first record of an operator== run (every record without duplicate removal) counts
    // the run under its barcode; the run's last record has its largest MAPQ, the survivor's under either rule.  Both mates of a pair are
    // records here: the writer halves these counts for paired-end data (SummaryMetadata::AdjustPairedEndOverCount)
    const uint64_t b = bc ? bc[i] : 0;
    bool head = !cfg.dedup || j == 0;
    if (!head) { const uint32_t i0 = idx[j - 1]; head = !sp_same_run(sp_load(rec, i0), bc ? bc[i0] : 0, r, b); }
    if (head) {
      uint32_t d = 1, mq = r.mapq;
      for (uint32_t t = j + 1; cfg.dedup && t < n; ++t, ++d) {
        const uint32_t i2 = idx[t];
        const SpRec nx = sp_load(rec, i2);
        if (!sp_same_run(nx, bc ? bc[i2] : 0, r, b)) break;
        mq = nx.mapq;
      }
      if (cfg.dedup == 2 && d > 255) d = 255;
      cm_sm_credit(sm, bc == nullptr, b, d, (int)mq >= cfg.mapq_thr);
    }
  }
  if ((int)r.mapq < cfg.mapq_thr || r.rid >= cfg.n_seq) { line_len[j] = 0; return; }
  // --remove-pcr-duplicates: one survivor per run of operator==; the records stand in operator< order, inside a run by (mapq, read_id).
  // The filter above is the survivor's: it has the run's largest MAPQ under either rule, and rid / mrid are the run's.
  if (cfg.dedup) {
    const uint64_t b = bc ? bc[i] : 0;
    bool win;
    if (cfg.dedup == 2) {
      win = j + 1 == n;
      if (!win) { const uint32_t i2 = idx[j + 1]; win = !sp_same_run(sp_load(rec, i2), bc ? bc[i2] : 0, r, b); }
    } else {
      win = j == 0;
      if (!win) { const uint32_t i0 = idx[j - 1]; const SpRec pr = sp_load(rec, i0); win = !sp_same_run(pr, bc ? bc[i0] : 0, r, b) || pr.mapq != r.mapq; }
      for (uint32_t t = j + 1; win && t < n; ++t) {
        const uint32_t i2 = idx[t];
        const SpRec nx = sp_load(rec, i2);
        if (!sp_same_run(nx, bc ? bc[i2] : 0, r, b)) break;
        if (nx.mapq != r.mapq) win = false;
      }
    }
    if (!win) { line_len[j] = 0; return; }
  }
  // the record is printed: only now does a barcode the translation table lacks count (the reference exits in Translate, which it
  // calls for a mapping it is about to print)
  uint32_t cb_len = cfg.bc_len;
  if (cfg.bc_len && cfg.bt.tab && !cm_bt_length(cfg.bt, bc[i], cfg.bc_len, &cb_len)) { atomicAdd(counts + 1, 1ull); line_len[j] = 0; return; }
  const uint32_t mate = r.valid - 1u;
  uint32_t cig_text;
  const uint32_t sl = sp_seq_len(r, reinterpret_cast<const uint32_t *>(var + var_offs[i]), &cig_text);
  const uint32_t nm_len = (uint32_t)(rs.name_offs[mate][q + 1] - rs.name_offs[mate][q]);
  if (BAM) {
    if (nm_len > CM_BAM_NAME_MAX) { atomicAdd(counts + 2, 1ull); line_len[j] = 0; return; }
    line_len[j] = cm_bam_record_size(r, reinterpret_cast<const uint32_t *>(var + var_offs[i]), nm_len, cfg.bc_len != 0, cb_len);
    return;
  }
  const uint32_t rnext = r.mrid < 0 || (uint32_t)r.mrid == r.rid ? 1u : name_off[r.mrid + 1] - name_off[r.mrid];
  const uint32_t tl = r.tlen < 0 ? 1u + cm_digits10((uint32_t)(-(int64_t)r.tlen)) : cm_digits10((uint32_t)r.tlen);
  line_len[j] = (uint64_t)nm_len + 1 + cm_digits10(r.flag) + 1 + (name_off[r.rid + 1] - name_off[r.rid]) + 1 + cm_digits10(r.pos + 1) + 1 + cm_digits10(r.mapq) + 1 +
                cig_text + 1 + rnext + 1 + cm_digits10(r.mrid < 0 ? 0u : r.mpos + 1) + 1 + tl + 1 + sl + 1 + sl + 6 + cm_digits10(r.nm) + 6 + r.md_len +
                (cfg.bc_len ? 6 + cb_len : 0) + 1;
}

// the group's lanes copy len bytes to dst: single bytes up to dst's next 4-byte boundary, then whole words, a word per lane and step (the
// source is read at whatever alignment it has), then the last bytes.  MODE 0: src[0 .. len) as it is; 1: reversed, src[len-1] first (the quality
// of a read on the - strand); 2: reversed and complemented (its bases: Uint8ToChar(3 ^ CharToUint8(c)), anything but ACGT gives N)
__device__ __forceinline__ uint32_t sp_comp(uint32_t c) {
  const uint32_t u = c & 0xDFu;
  return u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : u == 'T' ? 'A' : 'N';
}
template <int MODE>
__device__ __forceinline__ uint32_t sp_byte(const uint8_t *__restrict__ src, uint32_t len, uint32_t t) {
  return MODE == 0 ? src[t] : MODE == 1 ? src[len - 1u - t] : sp_comp(src[len - 1u - t]);
}
template <int MODE, int G>
__device__ __forceinline__ void sp_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint32_t len, uint32_t lane) {
  uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
  if (head > len) head = len;
  if (lane < head) dst[lane] = (uint8_t)sp_byte<MODE>(src, len, lane);
  const uint32_t words = (len - head) / 4u;
  for (uint32_t w = lane; w < words; w += G) {
    const uint32_t t = head + 4u * w;
    uint32_t x;
    if (MODE == 0) __builtin_memcpy(&x, src + t, 4);
    else {
      __builtin_memcpy(&x, src + (len - 4u - t), 4);  // bytes len-4-t .. len-1-t; the last of them goes first
      x = __builtin_bswap32(x);
      if (MODE == 2) x = sp_comp(x & 0xffu) | (sp_comp((x >> 8) & 0xffu) << 8) | (sp_comp((x >> 16) & 0xffu) << 16) | (sp_comp(x >> 24) << 24);
    }
    *reinterpret_cast<uint32_t *>(dst + t) = x;
  }
  const uint32_t t = head + 4u * words + lane;
  if (t < len) dst[t] = (uint8_t)sp_byte<MODE>(src, len, t);
}
// G lanes per line (G = 8, 16 or 64 -- a divisor of the block).  Every lane works out where the columns start (a few loads the whole group
// shares); lane 0 writes the numeric columns, the CIGAR and the tags' values, the group copies the read's name, the reference names, SEQ, QUAL and MD.
template <int G>
__global__ __launch_bounds__(SP_BLOCK) void k_sp_format(const uint8_t *__restrict__ rec, const uint64_t *__restrict__ bc, const uint8_t *__restrict__ var,
                                                          const uint64_t *__restrict__ var_offs, const uint32_t *__restrict__ idx, uint32_t n, SpCfg cfg,
                                                          SpReads rs, const uint8_t *__restrict__ names, const uint32_t *__restrict__ name_off,
                                                          const uint64_t *__restrict__ line_len, const uint64_t *__restrict__ line_off,
                                                          uint8_t *__restrict__ text) {
  const uint64_t jj = ((uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x) / G;
  const uint32_t j = (uint32_t)jj, lane = threadIdx.x % G;
  if (jj >= n || line_len[j] == 0) return;
  const uint32_t i = idx[j];
  const SpRec r = sp_load(rec, i);
  const uint32_t mate = r.valid - 1u;
  const uint64_t q = (uint64_t)(r.read_id - cfg.base);
  const uint32_t *cg = reinterpret_cast<const uint32_t *>(var + var_offs[i]);
  const uint8_t *md = reinterpret_cast<const uint8_t *>(cg + r.n_cigar);
  uint32_t cig_text;
  const uint32_t sl = sp_seq_len(r, cg, &cig_text), L = r.trim_len;
  const uint64_t no = rs.name_offs[mate][q], ro = rs.offs[mate][q];
  const uint32_t nm_len = (uint32_t)(rs.name_offs[mate][q + 1] - no);
  const uint32_t rn0 = name_off[r.rid], rn1 = name_off[r.rid + 1];
  const bool other = r.mrid >= 0 && (uint32_t)r.mrid != r.rid;
  const uint32_t mn0 = other ? name_off[r.mrid] : 0u, mn1 = other ? name_off[r.mrid + 1] : 1u;
  const uint32_t pnext = r.mrid < 0 ? 0u : r.mpos + 1u;
  const uint32_t tl = r.tlen < 0 ? 1u + cm_digits10((uint32_t)(-(int64_t)r.tlen)) : cm_digits10((uint32_t)r.tlen);
  uint8_t *line = text + line_off[j];
  uint8_t *mid = line + nm_len;  // '\t' FLAG ... TLEN '\t'
  const uint32_t mid_len = 1 + cm_digits10(r.flag) + 1 + (rn1 - rn0) + 1 + cm_digits10(r.pos + 1) + 1 + cm_digits10(r.mapq) + 1 + cig_text + 1 + (mn1 - mn0) + 1 +
                           cm_digits10(pnext) + 1 + tl + 1;
  uint8_t *seq = mid + mid_len, *qual = seq + sl + 1, *tail = qual + sl;
  sp_copy<0, G>(line, rs.names[mate] + no, nm_len, lane);
  // the printed bases are the first sl of the L mapped ones as they stand in the SAM line: on the - strand the line starts at the read's base L - 1
  const uint8_t *bs = rs.bases[mate] + ro, *qs = rs.quals[mate] + ro;
  if (r.strand) { sp_copy<0, G>(seq, bs, sl, lane); sp_copy<0, G>(qual, qs, sl, lane); }
  else { sp_copy<2, G>(seq, bs + (L - sl), sl, lane); sp_copy<1, G>(qual, qs + (L - sl), sl, lane); }
  sp_copy<0, G>(tail + 6 + cm_digits10(r.nm) + 6, md, r.md_len, lane);
  uint8_t *rname_at = mid + 1 + cm_digits10(r.flag) + 1;
  sp_copy<0, G>(rname_at, names + rn0, rn1 - rn0, lane);
  if (other) sp_copy<0, G>(rname_at + (rn1 - rn0) + 1 + cm_digits10(r.pos + 1) + 1 + cm_digits10(r.mapq) + 1 + cig_text + 1, names + mn0, mn1 - mn0, lane);
  if (cfg.bc_len && cfg.bt.tab) {  // the translated CB:Z: value: the group copies the `to` strings, lane 0 puts the dashes between them
    uint8_t *d = tail + 6 + cm_digits10(r.nm) + 6 + r.md_len + 6;
    const uint64_t key = bc[i];
    const uint32_t nseg = cfg.bc_len / cfg.bt.from_len;
    for (uint32_t sg = 0; sg < nseg; ++sg) {
      if (sg) { if (lane == 0) *d = '-'; ++d; }
      const uint64_t v = cm_bt_find(cfg.bt, cm_bt_seed(cfg.bt, key, nseg, sg));
      if (v == CM_BT_EMPTY) continue;
      sp_copy<0, G>(d, cfg.bt.blob + (v >> 32), (uint32_t)v, lane);
      d += (uint32_t)v;
    }
  }
  if (lane == 0) {
    uint8_t *p = mid;
    *p++ = '\t';
    p = cm_put_u32(p, r.flag);
    *p++ = '\t';
    p += rn1 - rn0;  // (RNAME: the group's copy above)
    *p++ = '\t';
    p = cm_put_u32(p, r.pos + 1);
    *p++ = '\t';
    p = cm_put_u32(p, r.mapq);
    *p++ = '\t';
    if (r.n_cigar == 0) *p++ = '*';
    for (uint32_t t = 0; t < r.n_cigar; ++t) { p = cm_put_u32(p, cg[t] >> 4); *p++ = "MIDNSHP=XB??????"[cg[t] & 0xfu]; }
    *p++ = '\t';
    if (r.mrid < 0) *p++ = '*';
    else if (!other) *p++ = '=';
    else p += mn1 - mn0;  // (RNEXT by name: the group's copy above)
    *p++ = '\t';
    p = cm_put_u32(p, pnext);
    *p++ = '\t';
    if (r.tlen < 0) { *p++ = '-'; p = cm_put_u32(p, (uint32_t)(-(int64_t)r.tlen)); } else p = cm_put_u32(p, (uint32_t)r.tlen);
    *p++ = '\t';
    seq[sl] = '\t';
    p = tail;
    *p++ = '\t'; *p++ = 'N'; *p++ = 'M'; *p++ = ':'; *p++ = 'i'; *p++ = ':';
    p = cm_put_u32(p, r.nm);
    *p++ = '\t'; *p++ = 'M'; *p++ = 'D'; *p++ = ':'; *p++ = 'Z'; *p++ = ':';
    p += r.md_len;
    if (cfg.bc_len) {
      *p++ = '\t'; *p++ = 'C'; *p++ = 'B'; *p++ = ':'; *p++ = 'Z'; *p++ = ':';
      if (cfg.bt.tab) p = line + line_len[j] - 1;  // (the value: the group's copy above)
      else {
        const uint64_t key = bc[i];
        for (uint32_t b = 0; b < cfg.bc_len; ++b) *p++ = "ACGT"[(key >> ((cfg.bc_len - 1 - b) * 2)) & 3];  // Seed2Sequence
      }
    }
    *p = '\n';
  }
}

// The same G lanes per selected record, which becomes a BAM alignment record (cm_bam.h: cm_bam_encode) at its offset: lane 0 writes the
// fixed 36 bytes and the tags' heads, the group name, CIGAR, SEQ, QUAL, MD and the barcode.  A translated CB:Z value is copied here, as in
// k_sp_format.
template <int G_>
struct SpLanes {
  static constexpr int G = G_;
  uint32_t t;
};
template <int G>
__global__ __launch_bounds__(SP_BLOCK) void k_bam_format(const uint8_t *__restrict__ rec, const uint64_t *__restrict__ bc, const uint8_t *__restrict__ var,
                                                           const uint64_t *__restrict__ var_offs, const uint32_t *__restrict__ idx, uint32_t n, SpCfg cfg,
                                                           SpReads rs, const uint64_t *__restrict__ rec_len, const uint64_t *__restrict__ rec_off,
                                                           uint8_t *__restrict__ out) {
  const uint64_t jj = ((uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x) / G;
  const uint32_t j = (uint32_t)jj;
  if (jj >= n || rec_len[j] == 0) return;
  SpLanes<G> g;
  g.t = threadIdx.x % G;
  const uint32_t i = idx[j];
  const SpRec r = sp_load(rec, i);
  const uint32_t mate = r.valid - 1u;
  const uint64_t q = (uint64_t)(r.read_id - cfg.base);
  const uint32_t *cg = reinterpret_cast<const uint32_t *>(var + var_offs[i]);
  const uint8_t *md = reinterpret_cast<const uint8_t *>(cg + r.n_cigar);
  const uint64_t no = rs.name_offs[mate][q], ro = rs.offs[mate][q];
  const uint32_t nm_len = (uint32_t)(rs.name_offs[mate][q + 1] - no);
  const bool has_cb = cfg.bc_len != 0, plain = cfg.bt.tab == nullptr;
  const uint64_t key = has_cb ? bc[i] : 0;
  uint32_t cb_len = cfg.bc_len;
  if (has_cb && !plain) (void)cm_bt_length(cfg.bt, key, cfg.bc_len, &cb_len);  // (k_sp_len selected the record: every segment is in the table)
  uint8_t *d = cm_bam_encode(g, out + rec_off[j], r, cg, md, rs.names[mate] + no, nm_len, rs.bases[mate] + ro, rs.quals[mate] + ro, has_cb, cb_len, plain, key);
  if (has_cb && !plain) {  // the `to` strings by the group, the dashes between them by lane 0
    const uint32_t nseg = cfg.bc_len / cfg.bt.from_len;
    for (uint32_t sg = 0; sg < nseg; ++sg) {
      if (sg) { if (g.t == 0) *d = '-'; ++d; }
      const uint64_t v = cm_bt_find(cfg.bt, cm_bt_seed(cfg.bt, key, nseg, sg));
      if (v == CM_BT_EMPTY) continue;
      cm_bam_spread(g, d, (uint32_t)v, CmBamBytes{cfg.bt.blob + (v >> 32)});
      d += (uint32_t)v;
    }
  }
}

// both writers: the sort, the selection (k_sp_len) and the checks are one; bam: the selected records' lengths and the format kernel are BAM's
static int sp_format_store(cmgpu_ctx *c, const char *const *ref_names, uint32_t n_sequences, const cmgpu_params *p, uint32_t barcode_length, bool bam,
                           uint64_t *n_lines, uint64_t *n_bytes) {
  if (!c || !ref_names || !p || !n_lines || !n_bytes) return CMGPU_EINVAL;
  if (p->allocate_multi_mappings && !p->low_memory_mode) { cm_set_error(c, "allocate_multi_mappings: SAM records have no allocation stage"); return CMGPU_EINVAL; }
  CM_HIPCHECK(c, cm_enter(c));
  CmSamStore &st = c->ss;
  if (st.has_bc && (barcode_length == 0 || barcode_length > 32)) { cm_set_error(c, "the SAM record store holds barcodes: barcode_length must be 1..32"); return CMGPU_EINVAL; }
  hipStream_t s = c->stream;
  *n_lines = 0;
  *n_bytes = 0;
  c->text_bytes = 0;
  c->text_lines = 0;
  c->bam_starts_have = false;  // (kept starts are those of one rendering: cmgpu_bam_keep_starts)
  const uint32_t n = (uint32_t)st.n;
  if (n == 0) return bam && c->bam_keep ? cm_bai_keep_starts(c, nullptr, nullptr, 0, 0, 0) : CMGPU_OK;
  if (c->rd_n == 0 || (st.paired && !c->rd_paired)) { cm_set_error(c, "the read store is empty: SAM text needs the reads of the run (cmgpu_fastq_keep_reads)"); return CMGPU_EINVAL; }
  CmTextJob job;
  int rc;
  if ((rc = job.begin(c, ref_names, n_sequences, n, 2, true))) return rc;
  const dim3 g((n + SP_BLOCK - 1) / SP_BLOCK), b(SP_BLOCK);
  const uint8_t *rec = (const uint8_t *)st.rec.p;
  const uint64_t *bc = st.has_bc ? (const uint64_t *)st.bc.p : (const uint64_t *)nullptr;
  // least significant key first, stable passes: (mapq, read_id), (mpos, flag & 64), mrid, barcode, (rid, pos)
  const unsigned bits[5] = {40, 33, job.rid_bits, st.has_bc ? 2 * barcode_length : 0, 32 + job.rid_bits};
  bool have_idx = false;
  for (int which = 0; which < 5; ++which) {
    if (bits[which] == 0) continue;
    hipLaunchKernelGGL(k_sp_key, g, b, 0, s, rec, bc, have_idx ? (const uint32_t *)job.idx() : (const uint32_t *)nullptr, n, which, n_sequences, job.keys(),
                       have_idx ? (uint32_t *)nullptr : job.idx());
    if ((rc = job.sort_pass(bits[which]))) return rc;
    have_idx = true;
  }
  SpCfg cfg;
  cfg.n_seq = n_sequences; cfg.bc_len = st.has_bc ? barcode_length : 0; cfg.base = c->rd_base; cfg.n_reads = c->rd_n;
  cfg.mapq_thr = p->mapq_threshold; cfg.dedup = p->remove_pcr_duplicates ? (p->low_memory_mode ? 1 : 2) : 0;
  cfg.bt = st.has_bc ? cm_bt_dev(c) : CmBtDev{nullptr, nullptr, 0, 0};
  SpReads rs;
  for (int m = 0; m < 2; ++m) {
    const CmReadMate &r = c->rd[st.paired ? m : 0];
    rs.names[m] = (const uint8_t *)r.names.p; rs.bases[m] = (const uint8_t *)r.bases.p; rs.quals[m] = (const uint8_t *)r.quals.p;
    rs.name_offs[m] = (const uint64_t *)r.name_offs.p; rs.offs[m] = (const uint64_t *)r.offs.p;
  }
  // the job's spare count words: records that belong to no read of the read store, lines whose barcode the translation table lacks, and
  // BAM records whose read name is too long (k_sp_len)
  if ((rc = job.zero_counts())) return rc;
  CmSmDev sm;  // --summary: the length kernel credits every run to its barcode (the keys are in the table since their reads were counted)
  if ((rc = cm_summary_dev(c, 0, 0, !st.has_bc, &sm))) return rc;
#define SP_LEN(BAM)                                                                                                                                 \
  hipLaunchKernelGGL(k_sp_len<BAM>, g, b, 0, s, rec, bc, (const uint8_t *)st.var.p, (const uint64_t *)st.var_offs.p, (const uint32_t *)job.idx(), n, cfg, rs, \
                     job.seq_off(), (uint64_t *)job.llen.p, job.extra_word(), sm)
  if (bam) SP_LEN(true); else SP_LEN(false);
#undef SP_LEN
  uint64_t total = 0, lines = 0, foreign = 0, misses = 0, long_names = 0;
  if ((rc = job.scan_lines(&total, &lines, &foreign, &misses, &long_names))) return rc;
  if (foreign) {
    cm_set_error(c, std::to_string((unsigned long long)foreign) + " SAM records belong to no read of the read store (reads " + std::to_string(c->rd_base) + " .. " +
                        std::to_string((unsigned long long)c->rd_base + c->rd_n) + ") or to a mate sequence the reference does not have: the record store and the read store are not of one run");
    return CMGPU_EINVAL;
  }
  if (misses) { cm_set_error(c, CM_BT_MISS_MESSAGE); return CMGPU_EFORMAT; }  // (no text: text_bytes is 0 since the call began)
  if (long_names) {
    cm_set_error(c, std::to_string((unsigned long long)long_names) + " records have a read name of more than " + std::to_string(CM_BAM_NAME_MAX) +
                        " bytes, the longest a BAM record's l_read_name holds: no BAM records are written");
    return CMGPU_EFORMAT;
  }
  // (the sort's buffers go before the text comes: a realistic run's text is several GB)
  job.release_sort();
  if ((rc = job.alloc_text(total, std::string(bam ? "BAM records: " : "SAM text: ") + std::to_string((unsigned long long)total) + " bytes"))) return rc;
  const int G = c->opt.sam_group;
  const dim3 gf((unsigned)(((uint64_t)n * G + SP_BLOCK - 1) / SP_BLOCK));
#define SP_LAUNCH(W)                                                                                                                             \
  hipLaunchKernelGGL(k_sp_format<W>, gf, b, 0, s, rec, bc, (const uint8_t *)st.var.p, (const uint64_t *)st.var_offs.p, (const uint32_t *)job.idx(), n, cfg, rs, \
                     (const uint8_t *)job.names.p, job.seq_off(), (const uint64_t *)job.llen.p, (const uint64_t *)job.loff.p, (uint8_t *)c->text.p)
#define BAM_LAUNCH(W)                                                                                                                            \
  hipLaunchKernelGGL(k_bam_format<W>, gf, b, 0, s, rec, bc, (const uint8_t *)st.var.p, (const uint64_t *)st.var_offs.p, (const uint32_t *)job.idx(), n, cfg, rs, \
                     (const uint64_t *)job.llen.p, (const uint64_t *)job.loff.p, (uint8_t *)c->text.p)
  if (bam) { if (G == 16) BAM_LAUNCH(16); else if (G == 64) BAM_LAUNCH(64); else BAM_LAUNCH(8); }
  else if (G == 16) SP_LAUNCH(16); else if (G == 64) SP_LAUNCH(64); else SP_LAUNCH(8);
#undef BAM_LAUNCH
#undef SP_LAUNCH
  if ((rc = job.publish(total, lines, n_lines, n_bytes))) return rc;
  c->text_bam = bam;
  if (bam && c->bam_keep) return cm_bai_keep_starts(c, (const uint64_t *)job.llen.p, (const uint64_t *)job.loff.p, n, lines, total);
  return CMGPU_OK;
}
extern "C" int cmgpu_store_format_sam(cmgpu_ctx *c, const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const cmgpu_params *p,
                                      uint32_t barcode_length, uint64_t *n_lines, uint64_t *n_bytes) {
  (void)ref_lengths;  // (the @SQ lines are the caller's: cmgpu_write_sam_header)
  return sp_format_store(c, ref_names, n_sequences, p, barcode_length, false, n_lines, n_bytes);
}
// the same store, sort and selection; the text store then holds BAM alignment records back to back (the header: cmgpu_write_bam_header)
extern "C" int cmgpu_store_format_bam(cmgpu_ctx *c, const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const cmgpu_params *p,
                                      uint32_t barcode_length, uint64_t *n_records, uint64_t *n_bytes) {
  (void)ref_lengths;  // (l_ref is the header's)
  return sp_format_store(c, ref_names, n_sequences, p, barcode_length, true, n_records, n_bytes);
}

// the @SQ lines (mapping_writer.cc:312-322: OutputHeader of MappingWriter<SAMMapping>); the text follows with cmgpu_store_write_text(path, append = 1)
extern "C" int cmgpu_write_sam_header(const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const char *out_path) {
  if (!ref_names || !ref_lengths || !out_path) return CMGPU_EINVAL;
  FILE *f = fopen(out_path, "wb");
  if (!f) return CMGPU_EIO;
  bool ok = true;
  for (uint32_t i = 0; i < n_sequences; ++i) ok = fprintf(f, "@SQ\tSN:%s\tLN:%u\n", ref_names[i], ref_lengths[i]) > 0 && ok;
  ok = fclose(f) == 0 && ok;
  return ok ? CMGPU_OK : CMGPU_EIO;
}

// the BAM header before compression (SAM spec 4.2): magic, l_text and the @SQ lines above, n_ref, and per sequence l_name (NUL included),
// the name, l_ref.  The records follow as BGZF blocks (cmgpu_store_compress_text + cmgpu_bgzf_write)
extern "C" int cmgpu_write_bam_header(const char *const *ref_names, const uint32_t *ref_lengths, uint32_t n_sequences, const char *out_path) {
  if (!ref_names || !ref_lengths || !out_path) return CMGPU_EINVAL;
  std::string text, refs;
  auto put32 = [](std::string &to, uint32_t v) { for (int b = 0; b < 4; ++b) to.push_back((char)(v >> (8 * b))); };
  for (uint32_t i = 0; i < n_sequences; ++i) {
    text += std::string("@SQ\tSN:") + ref_names[i] + "\tLN:" + std::to_string(ref_lengths[i]) + "\n";
    put32(refs, (uint32_t)strlen(ref_names[i]) + 1u);
    refs.append(ref_names[i], strlen(ref_names[i]) + 1);
    put32(refs, ref_lengths[i]);
  }
  std::string head("BAM\1", 4);
  put32(head, (uint32_t)text.size());
  head += text;
  put32(head, n_sequences);
  head += refs;
  FILE *f = fopen(out_path, "wb");
  if (!f) return CMGPU_EIO;
  bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
  ok = fclose(f) == 0 && ok;
  return ok ? CMGPU_OK : CMGPU_EIO;
}

// the device code of this translation unit is loaded at the first launch of one of its kernels: context creation launches this empty one (cm_api.hip: cm_load_device_code)
__global__ void k_touch_sam_post() {}
void cm_touch_sam_post(hipStream_t s) { hipLaunchKernelGGL(k_touch_sam_post, dim3(1), dim3(1), 0, s); }
