// cm_tabix.hip -- the tabix index of the compressed store, built where the text and the blocks' offsets lie (cm_tabix.h has the
// rules and the per-item functions; cm_bgzf_out.hip leaves the text's whereabouts and the offset table).  Everything as long as the text,
// its lines or its raw chunks is a kernel, a scan or a sort on the context's stream; the host sees the number of lines, of references
// and of chunks, the references' table and names, and the finished arrays, which it writes out as the payload.
// Temporary device memory, all of it a CmTmpBuf released when the call returns: 24 bytes per line (start, begin, end, reference,
// raw chunk), 16 bytes per 4 KiB of text (the tiles' newline counts and their scan), 44 bytes per raw chunk (key and number twice
// for the sort, two virtual offsets, the merge flag), 24 per merged chunk, 8 per 16 kb window of every reference, 40 per reference
// and its name, and rocprim's work areas.
// The BAM index of a compressed chain of BAM records (cm_bai.h) is built here too: its keys come from the records' fields, and from
// the raw chunks on it is the same index -- the same kernels, scans and sort.  Its temporary memory: 16 bytes per record (begin, end,
// reference, raw chunk; the starts are kept by cmgpu_store_format_bam or uploaded: 8 more), 40 per reference, and the chunks' and
// windows' as above.
// The CSI index of either store (cm_tabix.h) runs the same kernels with its depth in the arrays and one more over the merged chunks
// (k_csi_loffset: 8 more bytes per merged chunk); its windows are not copied to the host -- chunks, the bins' loffsets and the
// references' table are.
#include <stdio.h>
#include <string.h>

#include <string>
#include <unordered_set>
#include <vector>

#include "cm_bai.h"
#include "cm_ctx.h"
#include "cm_tabix.h"
#include "cm_text_job.h"

#define TX_LANES 256

// the group type cm_tabix.h's tile functions ask for: the workgroup
struct TxGroup {
  static constexpr int G = TX_LANES;
  uint32_t t;
  uint32_t *xw;  // G / 64 words of shared memory: the waves' totals
  __device__ __forceinline__ uint32_t scan(uint32_t v, uint32_t *total) {
    const uint32_t wl = t & 63u, wv = t >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
      const uint32_t x = __shfl_up(incl, dlt, 64);
      if (wl >= (uint32_t)dlt) incl += x;
    }
    if (wl == 63u) xw[wv] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < G / 64; ++q) { const uint32_t x = xw[q]; base += (uint32_t)q < wv ? x : 0u; tot += x; }
    __syncthreads();
    *total = tot;
    return base + incl - v;
  }
  __device__ __forceinline__ uint32_t sum(uint32_t v) { uint32_t tot; (void)scan(v, &tot); return tot; }
};
struct TxAtomics {
  static __device__ __forceinline__ void min64(unsigned long long *p, unsigned long long v) { atomicMin(p, v); }
};

__global__ __launch_bounds__(TX_LANES) void k_tbx_count(const uint8_t *__restrict__ text, uint64_t n, uint64_t *__restrict__ cnt) {
  __shared__ uint32_t xw[TX_LANES / 64];
  TxGroup g;
  g.t = threadIdx.x;
  g.xw = xw;
  const uint32_t c = cm_tbx_tile_count(g, text, n, blockIdx.x);
  if (g.t == 0) cnt[blockIdx.x] = c;
}
__global__ __launch_bounds__(TX_LANES) void k_tbx_starts(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ first, uint64_t *__restrict__ lstart) {
  __shared__ uint32_t xw[TX_LANES / 64];
  TxGroup g;
  g.t = threadIdx.x;
  g.xw = xw;
  cm_tbx_tile_starts(g, text, n, blockIdx.x, first[blockIdx.x], lstart);
}
__global__ __launch_bounds__(TX_LANES) void k_tbx_parse(CmTbxArrays d) {
  const uint64_t i = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  if (i < d.n_lines) cm_tbx_line_parse<TxAtomics>(d, i);
}
// (no lane leaves early: the wave's lanes meet to raise their reference's n_intv with one atomic where they all have the same one)
__global__ __launch_bounds__(TX_LANES) void k_tbx_flags(CmTbxArrays d) {
  const uint64_t i = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  uint32_t t = ~0u, want = 0;
  unsigned long long e = CM_TBX_NO_ERROR;
  if (i < d.n_lines) want = cm_tbx_line_flags_core(d, i, &t, &e);
  if (e != CM_TBX_NO_ERROR) atomicMin(d.err, e);
  const uint32_t t0 = __shfl(t, 0, 64);
  if (__all(t == t0)) {
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) { const uint32_t x = __shfl_xor(want, dlt, 64); want = x > want ? x : want; }
    if ((threadIdx.x & 63u) == 0 && t != ~0u) atomicMax(&d.ref[t].n_intv, want);
  } else if (t != ~0u) {
    atomicMax(&d.ref[t].n_intv, want);
  }
}
__global__ __launch_bounds__(TX_LANES) void k_tbx_emit(CmTbxArrays d) {
  const uint64_t i = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  if (i < d.n_lines) cm_tbx_line_emit<TxAtomics>(d, i);
}
// reference r's name to blob + off[r]
__global__ __launch_bounds__(TX_LANES) void k_tbx_names(const uint8_t *__restrict__ text, const CmTbxRef *__restrict__ ref, const uint64_t *__restrict__ off, uint32_t n_ref,
                                                     uint8_t *__restrict__ blob) {
  const uint32_t r = blockIdx.x * TX_LANES + threadIdx.x;
  if (r >= n_ref) return;
  const uint8_t *src = text + ref[r].name_at;
  uint8_t *dst = blob + off[r];
  for (uint32_t i = 0; i < ref[r].name_len; ++i) dst[i] = src[i];
}
__global__ __launch_bounds__(TX_LANES) void k_tbx_chunk_flags(const uint64_t *__restrict__ key, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ cbeg,
                                                           const uint64_t *__restrict__ cend, uint64_t n, uint32_t *__restrict__ flag) {
  const uint64_t j = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  if (j < n) flag[j] = cm_tbx_chunk_flag(key, perm, cbeg, cend, j);
}
__global__ __launch_bounds__(TX_LANES) void k_tbx_chunk_emit(const uint64_t *__restrict__ key, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ cbeg,
                                                          const uint64_t *__restrict__ cend, const uint32_t *__restrict__ midx, uint64_t n, CmTbxChunk *__restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  if (j < n) cm_tbx_chunk_emit(key, perm, cbeg, cend, midx, n, j, out);
}
// the CSI's loffset of every bin, at the merged chunk that is the first of its (reference, bin): the back-filled window in which the
// bin begins.  (The other chunks' words are not read.)
__global__ __launch_bounds__(TX_LANES) void k_csi_loffset(const CmTbxChunk *__restrict__ ch, uint64_t n, uint32_t depth, const unsigned long long *__restrict__ lin,
                                                       const uint64_t *__restrict__ lin_off, uint64_t *__restrict__ loff) {
  const uint64_t j = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  if (j >= n) return;
  const uint64_t key = ch[j].key;
  loff[j] = j == 0 || ch[j - 1].key != key ? cm_csi_bin_loffset(key, depth, lin, lin_off) : 0ull;
}

// ---- the BAM index's per-record kernels (cm_bai.h): one lane per record
__global__ __launch_bounds__(TX_LANES) void k_bai_parse(CmBaiArrays d) {
  const uint64_t i = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  if (i < d.n_rec) cm_bai_rec_parse<TxAtomics>(d, i);
}
// (no lane leaves early: the wave's lanes meet to raise their reference's n_intv and counts with one atomic each where they all have
// the same reference)
__global__ __launch_bounds__(TX_LANES) void k_bai_flags(CmBaiArrays d) {
  const uint64_t i = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  uint32_t t = ~0u, want = 0, unm = 0;
  if (i < d.n_rec) want = cm_bai_rec_flags_core(d, i, &t, &unm);
  const uint32_t t0 = __shfl(t, 0, 64);
  if (__all(t == t0)) {
    const uint32_t n_unm = (uint32_t)__popcll(__ballot(t != ~0u && unm)), n_all = (uint32_t)__popcll(__ballot(t != ~0u));
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) { const uint32_t x = __shfl_xor(want, dlt, 64); want = x > want ? x : want; }
    if ((threadIdx.x & 63u) == 0 && t != ~0u) {
      atomicMax(&d.ref[t].n_intv, want);
      if (n_all - n_unm) atomicAdd(&d.ref[t].n_mapped, (unsigned long long)(n_all - n_unm));
      if (n_unm) atomicAdd(&d.ref[t].n_unmapped, (unsigned long long)n_unm);
    }
  } else if (t != ~0u) {
    atomicMax(&d.ref[t].n_intv, want);
    atomicAdd(unm ? &d.ref[t].n_unmapped : &d.ref[t].n_mapped, 1ull);
  }
}
__global__ __launch_bounds__(TX_LANES) void k_bai_emit(CmBaiArrays d) {
  const uint64_t i = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  if (i < d.n_rec) cm_bai_rec_emit<TxAtomics>(d, i);
}
// out[rank of i among the selected] = loff[i] for the records with a length: the starts of the records the BAM writer wrote
__global__ __launch_bounds__(TX_LANES) void k_bai_keep(const uint64_t *__restrict__ llen, const uint64_t *__restrict__ loff, const uint64_t *__restrict__ rank, uint64_t n,
                                                    uint64_t n_out, uint64_t *__restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * TX_LANES + threadIdx.x;
  if (i < n && llen[i] && rank[i] < n_out) out[rank[i]] = loff[i];
}

namespace {
struct TxJob {
  cmgpu_ctx *c;
  hipStream_t s;
  const char *name = "tabix index";  // the messages' first words
  uint32_t csi_depth = 0;  // 1 .. 6: a CSI of that depth is being built
  CmTmpBuf tmp;  // rocprim's work area
  ~TxJob() { (void)hipStreamSynchronize(s); }
  int enomem() { cm_set_error(c, std::string("out of device memory (") + name + ")"); return CMGPU_ENOMEM; }
  int fail(const char *what, hipError_t e) { cm_set_error(c, std::string(name) + ", " + what + ": " + hipGetErrorString(e)); return CMGPU_EHIP; }
  // flags -> 1 + (number of the run each entry lies in), in place
  int scan_flags(uint32_t *v, uint64_t n) {
    size_t tb = 0;
    (void)rocprim::inclusive_scan(nullptr, tb, v, v, (size_t)n, rocprim::plus<uint32_t>(), s);
    if (tmp.ensure(tb + 256)) return enomem();
    const hipError_t e = rocprim::inclusive_scan(tmp.p, tb, v, v, (size_t)n, rocprim::plus<uint32_t>(), s);
    return e == hipSuccess ? CMGPU_OK : fail("scan", e);
  }
  // every window takes the smallest value from itself to the end: an empty one (all ones) that of the next window a line overlaps
  int back_fill(unsigned long long *lin, uint64_t n) {
    auto rev = rocprim::make_reverse_iterator(lin + n);
    size_t tb = 0;
    (void)rocprim::inclusive_scan(nullptr, tb, rev, rev, (size_t)n, rocprim::minimum<unsigned long long>(), s);
    if (tmp.ensure(tb + 256)) return enomem();
    const hipError_t e = rocprim::inclusive_scan(tmp.p, tb, rev, rev, (size_t)n, rocprim::minimum<unsigned long long>(), s);
    return e == hipSuccess ? CMGPU_OK : fail("back-fill", e);
  }
  int format_error(unsigned long long word) {
    cm_set_error(c, "tabix index: line " + std::to_string((word >> 3) + 1) + " " +
                        (csi_depth ? cm_csi_tbx_cause((uint32_t)(word & 7u), csi_depth) : std::string(cm_tbx_cause((uint32_t)(word & 7u)))));
    return CMGPU_EFORMAT;
  }
};
static inline uint32_t tx_blocks(uint64_t n) { return (uint32_t)((n + TX_LANES - 1) / TX_LANES); }
}  // namespace

#define TX_CHECK(job, what, call)                                  \
  do {                                                             \
    const hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) return (job).fail(what, e_);             \
  } while (0)

// ---- 3. (all indexes) the n_raw raw chunks by (reference, bin), file order kept; neighbours joined; the merged chunks to the host.
// With job.csi_depth, and lin / lin_off the back-filled windows on the device: the bins' loffsets too (h_loff, one word per chunk)
static int tx_merge_chunks(TxJob &job, uint64_t *ckey, uint32_t *cval, const uint64_t *cbeg, const uint64_t *cend, uint32_t n_raw, uint64_t n_ref,
                           std::vector<CmTbxChunk> &h_ch, const unsigned long long *lin = nullptr, const uint64_t *lin_off = nullptr,
                           std::vector<uint64_t> *h_loff = nullptr) {
  hipStream_t s = job.s;
  CmTmpBuf skey, perm, mflag, merged, loff;
  struct Wait { hipStream_t s; ~Wait() { (void)hipStreamSynchronize(s); } } wait{s};  // (behind the buffers, as TxJob behind its caller's)
  h_ch.clear();
  if (h_loff) h_loff->clear();
  if (n_raw == 0) return CMGPU_OK;
  if (skey.ensure((size_t)n_raw * 8) || perm.ensure((size_t)n_raw * 4) || mflag.ensure((size_t)n_raw * 4)) return job.enomem();
  const unsigned key_shift = cm_tbx_key_shift_of(job.csi_depth);
  unsigned bits = key_shift;
  while (bits < 32 + key_shift && (1ull << (bits - key_shift)) < n_ref) ++bits;
  {
    size_t tb = 0;
    TX_CHECK(job, "sort", rocprim::radix_sort_pairs(nullptr, tb, ckey, (uint64_t *)skey.p, cval, (uint32_t *)perm.p, (size_t)n_raw, 0, bits, s));
    if (job.tmp.ensure(tb + 256)) return job.enomem();
    TX_CHECK(job, "sort", rocprim::radix_sort_pairs(job.tmp.p, tb, ckey, (uint64_t *)skey.p, cval, (uint32_t *)perm.p, (size_t)n_raw, 0, bits, s));
  }
  hipLaunchKernelGGL(k_tbx_chunk_flags, dim3(tx_blocks(n_raw)), dim3(TX_LANES), 0, s, (const uint64_t *)skey.p, (const uint32_t *)perm.p, cbeg, cend, (uint64_t)n_raw,
                     (uint32_t *)mflag.p);
  TX_CHECK(job, "merge", hipGetLastError());
  { const int rc = job.scan_flags((uint32_t *)mflag.p, n_raw); if (rc) return rc; }
  uint32_t n_merged = 0;
  TX_CHECK(job, "merge", hipMemcpyAsync(&n_merged, (uint32_t *)mflag.p + (n_raw - 1), 4, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "merge", cm_stream_sync(s));
  h_ch.resize(n_merged);
  if (merged.ensure((size_t)n_merged * sizeof(CmTbxChunk))) return job.enomem();
  hipLaunchKernelGGL(k_tbx_chunk_emit, dim3(tx_blocks(n_raw)), dim3(TX_LANES), 0, s, (const uint64_t *)skey.p, (const uint32_t *)perm.p, cbeg, cend,
                     (const uint32_t *)mflag.p, (uint64_t)n_raw, (CmTbxChunk *)merged.p);
  TX_CHECK(job, "merge", hipGetLastError());
  TX_CHECK(job, "merge", hipMemcpyAsync(h_ch.data(), merged.p, (size_t)n_merged * sizeof(CmTbxChunk), hipMemcpyDeviceToHost, s));
  if (h_loff) {
    h_loff->resize(n_merged);
    if (loff.ensure((size_t)n_merged * 8)) return job.enomem();
    hipLaunchKernelGGL(k_csi_loffset, dim3(tx_blocks(n_merged)), dim3(TX_LANES), 0, s, (const CmTbxChunk *)merged.p, (uint64_t)n_merged, job.csi_depth, lin, lin_off,
                       (uint64_t *)loff.p);
    TX_CHECK(job, "loffset", hipGetLastError());
    TX_CHECK(job, "loffset", hipMemcpyAsync(h_loff->data(), loff.p, (size_t)n_merged * 8, hipMemcpyDeviceToHost, s));
  }
  TX_CHECK(job, "merge", cm_stream_sync(s));
  return CMGPU_OK;
}

// csi_depth 0: the .tbi payload; 1 .. 6: the CSI payload (tabix flavour) of that depth
static int tx_index(cmgpu_ctx *c, const uint8_t *text, uint64_t n, uint64_t base, uint32_t csi_depth, std::vector<uint8_t> &payload) {
  if (n == 0) {
    if (csi_depth) {
      std::vector<uint8_t> aux;
      cm_csi_tabix_aux(0, nullptr, nullptr, aux);
      cm_csi_serialize(csi_depth, aux.data(), (uint32_t)aux.size(), nullptr, 0, nullptr, 0, nullptr, payload);
    } else {
      cm_tbx_serialize(nullptr, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, payload);
    }
    return CMGPU_OK;
  }
  hipStream_t s = c->stream;
  CmTmpBuf tcnt, toff, lstart, beg, end, tid, cidx, err, ref, name_off, names, lin_off, lin, ckey, cval, cbeg, cend;
  TxJob job;  // (declared behind the buffers: on every return it waits for the stream before they go)
  job.c = c;
  job.s = s;
  job.csi_depth = csi_depth;
  CmTbxArrays d = {};
  d.csi_depth = csi_depth;
  d.t.p = text;
  d.t.n = n;
  d.t.n_blocks = c->bgzf_blocks;
  d.t.coff = (const uint64_t *)c->bgzf_coff.p;
  d.t.base = base;
  // ---- 1. line starts
  const uint64_t n_tiles = (n + CM_TBX_TILE - 1) / CM_TBX_TILE;
  if (n_tiles > 0x7fffffffull) { cm_set_error(c, "tabix index: the text is too long (8 TiB and more)"); return CMGPU_EINVAL; }
  if (tcnt.ensure((n_tiles + 1) * 8) || toff.ensure((n_tiles + 1) * 8)) return job.enomem();
  TX_CHECK(job, "memset", hipMemsetAsync((uint64_t *)tcnt.p + n_tiles, 0, 8, s));
  hipLaunchKernelGGL(k_tbx_count, dim3((uint32_t)n_tiles), dim3(TX_LANES), 0, s, text, n, (uint64_t *)tcnt.p);
  TX_CHECK(job, "line count", hipGetLastError());
  { const int rc = cm_scan_u64(c, (const uint64_t *)tcnt.p, (uint64_t *)toff.p, (size_t)n_tiles + 1, job.tmp, s, "tabix index"); if (rc) return rc; }
  uint64_t n_lines = 0;
  uint8_t last = 0;
  TX_CHECK(job, "line count", hipMemcpyAsync(&n_lines, (uint64_t *)toff.p + n_tiles, 8, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "line count", hipMemcpyAsync(&last, text + n - 1, 1, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "line count", cm_stream_sync(s));
  if (last != '\n') {
    cm_set_error(c, "tabix index: the text does not end with a newline (line " + std::to_string(n_lines + 1) + " is not complete)");
    return CMGPU_EFORMAT;
  }
  if (n_lines > CM_TBX_MAX_LINES) { cm_set_error(c, "tabix index: more than 2^32 - 2 lines"); return CMGPU_EINVAL; }
  if (lstart.ensure((n_lines + 1) * 8) || beg.ensure(n_lines * 4) || end.ensure(n_lines * 4) || tid.ensure(n_lines * 4) || cidx.ensure(n_lines * 4) ||
      err.ensure(8)) return job.enomem();
  d.n_lines = n_lines;
  d.lstart = (const uint64_t *)lstart.p;
  d.beg = (uint32_t *)beg.p;
  d.end = (uint32_t *)end.p;
  d.tid = (uint32_t *)tid.p;
  d.cidx = (uint32_t *)cidx.p;
  d.err = (unsigned long long *)err.p;
  TX_CHECK(job, "memset", hipMemsetAsync(lstart.p, 0, 8, s));
  TX_CHECK(job, "memset", hipMemsetAsync(err.p, 0xff, 8, s));
  hipLaunchKernelGGL(k_tbx_starts, dim3((uint32_t)n_tiles), dim3(TX_LANES), 0, s, text, n, (const uint64_t *)toff.p, (uint64_t *)lstart.p);
  TX_CHECK(job, "line starts", hipGetLastError());
  // ---- 2. per line: columns, names' runs
  hipLaunchKernelGGL(k_tbx_parse, dim3(tx_blocks(n_lines)), dim3(TX_LANES), 0, s, d);
  TX_CHECK(job, "columns", hipGetLastError());
  { const int rc = job.scan_flags(d.tid, n_lines); if (rc) return rc; }
  uint32_t n_ref = 0;
  unsigned long long word = CM_TBX_NO_ERROR;
  TX_CHECK(job, "columns", hipMemcpyAsync(&n_ref, d.tid + (n_lines - 1), 4, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "columns", hipMemcpyAsync(&word, d.err, 8, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "columns", cm_stream_sync(s));
  tcnt.release();
  toff.release();
  if (word != CM_TBX_NO_ERROR) return job.format_error(word);
  // references, sortedness, raw chunks' heads
  if (ref.ensure((size_t)n_ref * sizeof(CmTbxRef))) return job.enomem();
  d.ref = (CmTbxRef *)ref.p;
  TX_CHECK(job, "memset", hipMemsetAsync(ref.p, 0, (size_t)n_ref * sizeof(CmTbxRef), s));
  hipLaunchKernelGGL(k_tbx_flags, dim3(tx_blocks(n_lines)), dim3(TX_LANES), 0, s, d);
  TX_CHECK(job, "references", hipGetLastError());
  { const int rc = job.scan_flags(d.cidx, n_lines); if (rc) return rc; }
  uint32_t n_raw = 0;
  std::vector<CmTbxRef> h_ref(n_ref);
  TX_CHECK(job, "references", hipMemcpyAsync(&n_raw, d.cidx + (n_lines - 1), 4, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "references", hipMemcpyAsync(&word, d.err, 8, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "references", hipMemcpyAsync(h_ref.data(), ref.p, (size_t)n_ref * sizeof(CmTbxRef), hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "references", cm_stream_sync(s));
  if (word != CM_TBX_NO_ERROR) return job.format_error(word);
  // (host, per reference: where its name and its windows go)
  std::vector<uint64_t> h_name_off((size_t)n_ref + 1, 0), h_lin_off((size_t)n_ref + 1, 0);
  for (uint32_t r = 0; r < n_ref; ++r) {
    h_name_off[r + 1] = h_name_off[r] + h_ref[r].name_len;
    h_lin_off[r + 1] = h_lin_off[r] + h_ref[r].n_intv;
  }
  const uint64_t n_win = h_lin_off[n_ref], name_bytes = h_name_off[n_ref];
  if (name_off.ensure(((size_t)n_ref + 1) * 8) || names.ensure(name_bytes + 16) || lin_off.ensure(((size_t)n_ref + 1) * 8) || lin.ensure(n_win * 8 + 16) ||
      ckey.ensure((size_t)n_raw * 8) || cval.ensure((size_t)n_raw * 4) || cbeg.ensure((size_t)n_raw * 8) || cend.ensure((size_t)n_raw * 8)) return job.enomem();
  TX_CHECK(job, "upload", hipMemcpyAsync(name_off.p, h_name_off.data(), h_name_off.size() * 8, hipMemcpyHostToDevice, s));
  TX_CHECK(job, "upload", hipMemcpyAsync(lin_off.p, h_lin_off.data(), h_lin_off.size() * 8, hipMemcpyHostToDevice, s));
  TX_CHECK(job, "memset", hipMemsetAsync(lin.p, 0xff, n_win * 8, s));
  d.lin_off = (const uint64_t *)lin_off.p;
  d.lin = (unsigned long long *)lin.p;
  d.ckey = (uint64_t *)ckey.p;
  d.cbeg = (uint64_t *)cbeg.p;
  d.cend = (uint64_t *)cend.p;
  d.cval = (uint32_t *)cval.p;
  hipLaunchKernelGGL(k_tbx_names, dim3(tx_blocks(n_ref)), dim3(TX_LANES), 0, s, text, (const CmTbxRef *)ref.p, (const uint64_t *)name_off.p, n_ref, (uint8_t *)names.p);
  TX_CHECK(job, "names", hipGetLastError());
  hipLaunchKernelGGL(k_tbx_emit, dim3(tx_blocks(n_lines)), dim3(TX_LANES), 0, s, d);
  TX_CHECK(job, "raw chunks", hipGetLastError());
  { const int rc = job.back_fill(d.lin, n_win); if (rc) return rc; }
  std::vector<uint8_t> h_names(name_bytes + 1);
  std::vector<uint64_t> h_lin(csi_depth ? 1 : n_win + 1);  // (a CSI's windows stay on the device)
  TX_CHECK(job, "names", hipMemcpyAsync(h_names.data(), names.p, name_bytes, hipMemcpyDeviceToHost, s));
  if (!csi_depth) TX_CHECK(job, "names", hipMemcpyAsync(h_lin.data(), lin.p, n_win * 8, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "names", cm_stream_sync(s));
  // a name twice: its second run's first line is the offender (host: as many steps as there are references)
  {
    std::unordered_set<std::string> seen;
    for (uint32_t r = 0; r < n_ref; ++r)
      if (!seen.emplace((const char *)h_names.data() + h_name_off[r], (size_t)h_ref[r].name_len).second)
        return job.format_error((unsigned long long)h_ref[r].first_line << 3 | CM_TBX_E_RECUR);
  }
  // ---- 3. raw chunks by (reference, bin), file order kept; neighbours joined
  std::vector<CmTbxChunk> h_ch;
  std::vector<uint64_t> h_loff;
  {
    const int rc = tx_merge_chunks(job, d.ckey, d.cval, d.cbeg, d.cend, n_raw, n_ref, h_ch, d.lin, d.lin_off, csi_depth ? &h_loff : nullptr);
    if (rc) return rc;
  }
  // ---- 4. the payload
  if (csi_depth) {
    std::vector<uint8_t> aux;
    cm_csi_tabix_aux(n_ref, h_names.data(), h_name_off.data(), aux);
    std::vector<CmCsiRef> cref(n_ref);
    for (uint32_t r = 0; r < n_ref; ++r)
      cref[r] = CmCsiRef{h_ref[r].vbeg, h_ref[r].vend, (r + 1 < n_ref ? h_ref[r + 1].first_line : n_lines) - h_ref[r].first_line, 0, 1u, 0u};
    cm_csi_serialize(csi_depth, aux.data(), (uint32_t)aux.size(), cref.data(), n_ref, h_ch.data(), h_ch.size(), h_loff.data(), payload);
    return CMGPU_OK;
  }
  cm_tbx_serialize(h_ref.data(), n_ref, n_lines, h_names.data(), h_name_off.data(), h_ch.data(), h_ch.size(), h_lin.data(), h_lin_off.data(), payload);
  return CMGPU_OK;
}

// The BAM index of the n bytes of records at p, record i at starts[i] (device memory, n_rec + 1 entries)
// csi_depth 0: the .bai's bytes; 1 .. 6: the CSI payload (BAM flavour) of that depth
static int bai_index(cmgpu_ctx *c, const uint8_t *p, uint64_t n, uint64_t base, uint32_t n_ref, const uint64_t *starts, uint64_t n_rec, uint32_t csi_depth,
                     std::vector<uint8_t> &payload) {
  hipStream_t s = c->stream;
  CmTmpBuf beg, end, tid, cidx, err, ref, lin_off, lin, ckey, cval, cbeg, cend;
  TxJob job;  // (declared behind the buffers: on every return it waits for the stream before they go)
  job.c = c;
  job.s = s;
  job.name = "BAM index";
  job.csi_depth = csi_depth;
  std::vector<CmBaiRef> h_ref(n_ref);
  std::vector<uint64_t> h_lin_off((size_t)n_ref + 1, 0), h_lin(1), h_loff;
  std::vector<CmTbxChunk> h_ch;
  // the payload from the host's arrays
  auto serialize = [&]() {
    if (!csi_depth) { cm_bai_serialize(h_ref.data(), n_ref, h_ch.data(), h_ch.size(), h_lin.data(), h_lin_off.data(), payload); return; }
    std::vector<CmCsiRef> cref(n_ref);
    for (uint32_t r = 0; r < n_ref; ++r)
      cref[r] = CmCsiRef{h_ref[r].vbeg, h_ref[r].vend, h_ref[r].n_mapped, h_ref[r].n_unmapped, h_ref[r].n_intv ? 1u : 0u, 0u};
    cm_csi_serialize(csi_depth, nullptr, 0, cref.data(), n_ref, h_ch.data(), h_ch.size(), h_loff.data(), payload);
  };
  if (n_rec == 0) {
    if (n) { cm_set_error(c, "BAM index: " + std::to_string((unsigned long long)n) + " bytes and no record"); return CMGPU_EINVAL; }
    serialize();
    return CMGPU_OK;
  }
  if (n_rec > CM_BAI_MAX_RECORDS) { cm_set_error(c, "BAM index: more than 2^32 - 2 records"); return CMGPU_EINVAL; }
  CmBaiArrays d = {};
  d.csi_depth = csi_depth;
  d.t.p = p;
  d.t.n = n;
  d.t.n_blocks = c->bgzf_blocks;
  d.t.coff = (const uint64_t *)c->bgzf_coff.p;
  d.t.base = base;
  d.n_rec = n_rec;
  d.starts = starts;
  d.n_ref = n_ref;
  if (beg.ensure(n_rec * 4) || end.ensure(n_rec * 4) || tid.ensure(n_rec * 4) || cidx.ensure(n_rec * 4) || err.ensure(8) ||
      ref.ensure((size_t)n_ref * sizeof(CmBaiRef) + 16)) return job.enomem();
  d.beg = (uint32_t *)beg.p;
  d.end = (uint32_t *)end.p;
  d.tid = (uint32_t *)tid.p;
  d.cidx = (uint32_t *)cidx.p;
  d.err = (unsigned long long *)err.p;
  d.ref = (CmBaiRef *)ref.p;
  // ---- 1. per record: fields and checks
  TX_CHECK(job, "memset", hipMemsetAsync(err.p, 0xff, 8, s));
  TX_CHECK(job, "memset", hipMemsetAsync(ref.p, 0, (size_t)n_ref * sizeof(CmBaiRef), s));
  hipLaunchKernelGGL(k_bai_parse, dim3(tx_blocks(n_rec)), dim3(TX_LANES), 0, s, d);
  TX_CHECK(job, "records", hipGetLastError());
  unsigned long long word = CM_TBX_NO_ERROR;
  TX_CHECK(job, "records", hipMemcpyAsync(&word, d.err, 8, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "records", cm_stream_sync(s));
  if (word != CM_TBX_NO_ERROR) {
    cm_set_error(c, "BAM index: record " + std::to_string((word >> 3) + 1) + " " +
                        (csi_depth ? cm_csi_bai_cause((uint32_t)(word & 7u), csi_depth) : std::string(cm_bai_cause((uint32_t)(word & 7u)))));
    return CMGPU_EFORMAT;
  }
  // ---- 2. references, raw chunks' heads
  hipLaunchKernelGGL(k_bai_flags, dim3(tx_blocks(n_rec)), dim3(TX_LANES), 0, s, d);
  TX_CHECK(job, "references", hipGetLastError());
  { const int rc = job.scan_flags(d.cidx, n_rec); if (rc) return rc; }
  uint32_t n_raw = 0;
  TX_CHECK(job, "references", hipMemcpyAsync(&n_raw, d.cidx + (n_rec - 1), 4, hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "references", hipMemcpyAsync(h_ref.data(), ref.p, (size_t)n_ref * sizeof(CmBaiRef), hipMemcpyDeviceToHost, s));
  TX_CHECK(job, "references", cm_stream_sync(s));
  for (uint32_t r = 0; r < n_ref; ++r) h_lin_off[r + 1] = h_lin_off[r] + h_ref[r].n_intv;
  const uint64_t n_win = h_lin_off[n_ref];
  if (lin_off.ensure(((size_t)n_ref + 1) * 8) || lin.ensure(n_win * 8 + 16) || ckey.ensure((size_t)n_raw * 8) || cval.ensure((size_t)n_raw * 4) ||
      cbeg.ensure((size_t)n_raw * 8) || cend.ensure((size_t)n_raw * 8)) return job.enomem();
  TX_CHECK(job, "upload", hipMemcpyAsync(lin_off.p, h_lin_off.data(), h_lin_off.size() * 8, hipMemcpyHostToDevice, s));
  TX_CHECK(job, "memset", hipMemsetAsync(lin.p, 0xff, n_win * 8, s));
  d.lin_off = (const uint64_t *)lin_off.p;
  d.lin = (unsigned long long *)lin.p;
  d.ckey = (uint64_t *)ckey.p;
  d.cbeg = (uint64_t *)cbeg.p;
  d.cend = (uint64_t *)cend.p;
  d.cval = (uint32_t *)cval.p;
  hipLaunchKernelGGL(k_bai_emit, dim3(tx_blocks(n_rec)), dim3(TX_LANES), 0, s, d);
  TX_CHECK(job, "raw chunks", hipGetLastError());
  { const int rc = job.back_fill(d.lin, n_win); if (rc) return rc; }
  if (!csi_depth) {  // (a CSI's windows stay on the device)
    h_lin.resize(n_win + 1);
    TX_CHECK(job, "windows", hipMemcpyAsync(h_lin.data(), lin.p, n_win * 8, hipMemcpyDeviceToHost, s));
  }
  // ---- 3. raw chunks by (reference, bin), file order kept; neighbours joined
  {
    const int rc = tx_merge_chunks(job, d.ckey, d.cval, d.cbeg, d.cend, n_raw, n_ref, h_ch, d.lin, d.lin_off, csi_depth ? &h_loff : nullptr);
    if (rc) return rc;
  }
  // ---- 4. the payload
  serialize();
  return CMGPU_OK;
}
// cmgpu_store_format_bam, behind publish: the offsets of the records it wrote -- loff where llen != 0 -- and `total` behind them
int cm_bai_keep_starts(cmgpu_ctx *c, const uint64_t *llen, const uint64_t *loff, uint32_t n, uint64_t n_rec, uint64_t total) {
  hipStream_t s = c->stream;
  c->bam_starts_have = false;
  CmTmpBuf rank;
  TxJob job;
  job.c = c;
  job.s = s;
  job.name = "BAM record starts";
  if (c->bam_starts.ensure((n_rec + 1) * 8) || (n && rank.ensure((size_t)n * 8))) return job.enomem();
  if (n) {
    auto lines_in = rocprim::make_transform_iterator(llen, CmLinesOp());
    size_t tb = 0;
    (void)rocprim::exclusive_scan(nullptr, tb, lines_in, (uint64_t *)rank.p, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s);
    if (job.tmp.ensure(tb + 256)) return job.enomem();
    TX_CHECK(job, "scan", rocprim::exclusive_scan(job.tmp.p, tb, lines_in, (uint64_t *)rank.p, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s));
    hipLaunchKernelGGL(k_bai_keep, dim3(tx_blocks(n)), dim3(TX_LANES), 0, s, llen, loff, (const uint64_t *)rank.p, (uint64_t)n, n_rec, (uint64_t *)c->bam_starts.p);
    TX_CHECK(job, "compaction", hipGetLastError());
  }
  TX_CHECK(job, "upload", hipMemcpyAsync((uint64_t *)c->bam_starts.p + n_rec, &total, 8, hipMemcpyHostToDevice, s));
  TX_CHECK(job, "compaction", cm_stream_sync(s));
  c->bam_starts_have = true;
  c->bam_starts_n = n_rec;
  c->bam_starts_gen = c->text_gen;
  c->bam_starts_bytes = total;
  return CMGPU_OK;
}

// the text of the compressed store indexed: the .tbi payload (csi_depth 0) or the CSI's, into `payload`
static int tx_index_store(cmgpu_ctx *c, uint64_t base_offset, uint32_t csi_depth, std::vector<uint8_t> &payload) {
  const uint8_t *text = nullptr;
  switch (c->bgzf_src) {
    case CM_BZ_SRC_STORE:
      if (c->bgzf_text_gen != c->text_gen || c->bgzf_text_bytes != c->text_bytes) {
        cm_set_error(c, "tabix index: the text store has been rendered anew since it was compressed");
        return CMGPU_EINVAL;
      }
      if (c->text_bam) {
        cm_set_error(c, "tabix index: the text store holds BAM records, not BED lines (BAM takes a .bai index: cmgpu_bgzf_index_bai)");
        return CMGPU_EFORMAT;
      }
      text = static_cast<const uint8_t *>(c->text.p);
      break;
    case CM_BZ_SRC_UPLOAD: text = static_cast<const uint8_t *>(c->bgzf_in.p); break;
    case CM_BZ_SRC_DEVICE: text = c->bgzf_src_ptr; break;
    default:
      cm_set_error(c, "tabix index: no compressed store to index (cmgpu_bgzf_compress or cmgpu_store_compress_text comes first)");
      return CMGPU_EINVAL;
  }
  if (base_offset >> 47) { cm_set_error(c, "tabix index: base offset beyond 2^47"); return CMGPU_EINVAL; }
  return tx_index(c, text, c->bgzf_text_bytes, base_offset, csi_depth, payload);
}
extern "C" int cmgpu_bgzf_index_tabix(cmgpu_ctx *c, uint64_t base_offset, uint64_t *n_bytes) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  c->tabix.clear();
  c->tabix_have = false;
  if (n_bytes) *n_bytes = 0;
  std::vector<uint8_t> payload;
  const int rc = tx_index_store(c, base_offset, 0, payload);
  if (rc != CMGPU_OK) return rc;
  c->tabix.swap(payload);
  c->tabix_have = true;
  if (n_bytes) *n_bytes = c->tabix.size();
  return CMGPU_OK;
}
extern "C" int cmgpu_tabix_download(cmgpu_ctx *c, void *out, uint64_t capacity) {
  if (!c || !out) return CMGPU_EINVAL;
  if (!c->tabix_have) { cm_set_error(c, "no tabix index (cmgpu_bgzf_index_tabix comes first)"); return CMGPU_EINVAL; }
  if (capacity < c->tabix.size()) { cm_set_error(c, "tabix buffer too small"); return CMGPU_ECAPACITY; }
  memcpy(out, c->tabix.data(), c->tabix.size());
  return CMGPU_OK;
}
extern "C" int cmgpu_tabix_write(cmgpu_ctx *c, const char *path) {
  if (!c || !path) return CMGPU_EINVAL;
  if (!c->tabix_have) { cm_set_error(c, "no tabix index (cmgpu_bgzf_index_tabix comes first)"); return CMGPU_EINVAL; }
  if (cmgpu_bgzf_write_host_text(path, c->tabix.data(), c->tabix.size(), 0) != CMGPU_OK || cmgpu_bgzf_write_eof(path) != CMGPU_OK) {
    remove(path);
    cm_set_error(c, std::string("cannot write ") + path);
    return CMGPU_EIO;
  }
  return CMGPU_OK;
}

// ---- the BAM index
extern "C" int cmgpu_bam_keep_starts(cmgpu_ctx *c, int on) {
  if (!c) return CMGPU_EINVAL;
  c->bam_keep = on != 0;
  if (!on) c->bam_starts_have = false;
  return CMGPU_OK;
}
// the records of the compressed store indexed: the .bai's bytes (csi_depth 0) or the CSI's, into `payload`
static int bai_index_store(cmgpu_ctx *c, uint64_t base_offset, uint32_t n_ref, const uint64_t *starts, uint64_t n_records, uint32_t csi_depth,
                           std::vector<uint8_t> &payload) {
  const uint8_t *p = nullptr;
  switch (c->bgzf_src) {
    case CM_BZ_SRC_STORE:
      if (c->bgzf_text_gen != c->text_gen || c->bgzf_text_bytes != c->text_bytes) {
        cm_set_error(c, "BAM index: the text store has been rendered anew since it was compressed");
        return CMGPU_EINVAL;
      }
      p = static_cast<const uint8_t *>(c->text.p);
      break;
    case CM_BZ_SRC_UPLOAD: p = static_cast<const uint8_t *>(c->bgzf_in.p); break;
    case CM_BZ_SRC_DEVICE: p = c->bgzf_src_ptr; break;
    default:
      cm_set_error(c, "BAM index: no compressed store to index (cmgpu_bgzf_compress or cmgpu_store_compress_text comes first)");
      return CMGPU_EINVAL;
  }
  if (base_offset >> 47) { cm_set_error(c, "BAM index: base offset beyond 2^47"); return CMGPU_EINVAL; }
  const uint64_t n = c->bgzf_text_bytes;
  CmTmpBuf up;
  const uint64_t *d_starts = nullptr;
  if (!starts) {  // the starts cmgpu_store_format_bam kept: they belong to the rendering that was compressed
    if (c->bgzf_src != CM_BZ_SRC_STORE || !c->bam_starts_have || c->bam_starts_gen != c->text_gen || c->bam_starts_bytes != c->text_bytes) {
      cm_set_error(c, c->bgzf_src == CM_BZ_SRC_STORE && !c->text_bam && c->text_bytes
                          ? "BAM index: the text store does not hold BAM records (cmgpu_store_format_bam renders them)"
                          : "BAM index: no record starts were kept for the compressed store (cmgpu_bam_keep_starts comes before cmgpu_store_format_bam)");
      return CMGPU_EINVAL;
    }
    d_starts = (const uint64_t *)c->bam_starts.p;
    n_records = c->bam_starts_n;
  } else {
    if (n_records > CM_BAI_MAX_RECORDS) { cm_set_error(c, "BAM index: more than 2^32 - 2 records"); return CMGPU_EINVAL; }
    if (up.ensure((n_records + 1) * 8)) { cm_set_error(c, "out of device memory (BAM index)"); return CMGPU_ENOMEM; }
    CM_HIPCHECK(c, hipMemcpyAsync(up.p, starts, (n_records + 1) * 8, hipMemcpyHostToDevice, c->stream));
    CM_HIPCHECK(c, cm_stream_sync(c->stream));
    d_starts = (const uint64_t *)up.p;
  }
  return bai_index(c, p, n, base_offset, n_ref, d_starts, n_records, csi_depth, payload);
}
extern "C" int cmgpu_bgzf_index_bai(cmgpu_ctx *c, uint64_t base_offset, uint32_t n_ref, const uint64_t *starts, uint64_t n_records, uint64_t *n_bytes) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  c->bai.clear();
  c->bai_have = false;
  if (n_bytes) *n_bytes = 0;
  std::vector<uint8_t> payload;
  const int rc = bai_index_store(c, base_offset, n_ref, starts, n_records, 0, payload);
  if (rc != CMGPU_OK) return rc;
  c->bai.swap(payload);
  c->bai_have = true;
  if (n_bytes) *n_bytes = c->bai.size();
  return CMGPU_OK;
}
extern "C" int cmgpu_bai_download(cmgpu_ctx *c, void *out, uint64_t capacity) {
  if (!c || !out) return CMGPU_EINVAL;
  if (!c->bai_have) { cm_set_error(c, "no BAM index (cmgpu_bgzf_index_bai comes first)"); return CMGPU_EINVAL; }
  if (capacity < c->bai.size()) { cm_set_error(c, "BAM index buffer too small"); return CMGPU_ECAPACITY; }
  memcpy(out, c->bai.data(), c->bai.size());
  return CMGPU_OK;
}
extern "C" int cmgpu_bai_write(cmgpu_ctx *c, const char *path) {
  if (!c || !path) return CMGPU_EINVAL;
  if (!c->bai_have) { cm_set_error(c, "no BAM index (cmgpu_bgzf_index_bai comes first)"); return CMGPU_EINVAL; }
  FILE *f = fopen(path, "wb");
  bool ok = f != nullptr;
  if (f) {
    ok = fwrite(c->bai.data(), 1, c->bai.size(), f) == c->bai.size();
    ok = fclose(f) == 0 && ok;
  }
  if (!ok) {
    remove(path);
    cm_set_error(c, std::string("cannot write ") + path);
    return CMGPU_EIO;
  }
  return CMGPU_OK;
}

// ---- the CSI index: either store's, one payload
static int csi_begin(cmgpu_ctx *c, uint32_t depth, uint64_t *n_bytes) {
  c->csi.clear();
  c->csi_have = false;
  if (n_bytes) *n_bytes = 0;
  if (depth < 1 || depth > CM_CSI_MAX_DEPTH) { cm_set_error(c, "CSI index: depth must be 1 .. 6"); return CMGPU_EINVAL; }
  return CMGPU_OK;
}
static int csi_keep(cmgpu_ctx *c, std::vector<uint8_t> &payload, uint64_t *n_bytes) {
  c->csi.swap(payload);
  c->csi_have = true;
  if (n_bytes) *n_bytes = c->csi.size();
  return CMGPU_OK;
}
extern "C" int cmgpu_bgzf_index_csi_bam(cmgpu_ctx *c, uint64_t base_offset, uint32_t n_ref, const uint64_t *starts, uint64_t n_records, uint32_t depth,
                                        uint64_t *n_bytes) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  { const int rc = csi_begin(c, depth, n_bytes); if (rc) return rc; }
  std::vector<uint8_t> payload;
  const int rc = bai_index_store(c, base_offset, n_ref, starts, n_records, depth, payload);
  return rc != CMGPU_OK ? rc : csi_keep(c, payload, n_bytes);
}
extern "C" int cmgpu_bgzf_index_csi_tabix(cmgpu_ctx *c, uint64_t base_offset, uint32_t depth, uint64_t *n_bytes) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  { const int rc = csi_begin(c, depth, n_bytes); if (rc) return rc; }
  std::vector<uint8_t> payload;
  const int rc = tx_index_store(c, base_offset, depth, payload);
  return rc != CMGPU_OK ? rc : csi_keep(c, payload, n_bytes);
}
extern "C" int cmgpu_csi_download(cmgpu_ctx *c, void *out, uint64_t capacity) {
  if (!c || !out) return CMGPU_EINVAL;
  if (!c->csi_have) { cm_set_error(c, "no CSI index (cmgpu_bgzf_index_csi_bam or cmgpu_bgzf_index_csi_tabix comes first)"); return CMGPU_EINVAL; }
  if (capacity < c->csi.size()) { cm_set_error(c, "CSI index buffer too small"); return CMGPU_ECAPACITY; }
  memcpy(out, c->csi.data(), c->csi.size());
  return CMGPU_OK;
}
extern "C" int cmgpu_csi_write(cmgpu_ctx *c, const char *path) {
  if (!c || !path) return CMGPU_EINVAL;
  if (!c->csi_have) { cm_set_error(c, "no CSI index (cmgpu_bgzf_index_csi_bam or cmgpu_bgzf_index_csi_tabix comes first)"); return CMGPU_EINVAL; }
  if (cmgpu_bgzf_write_host_text(path, c->csi.data(), c->csi.size(), 0) != CMGPU_OK || cmgpu_bgzf_write_eof(path) != CMGPU_OK) {
    remove(path);
    cm_set_error(c, std::string("cannot write ") + path);
    return CMGPU_EIO;
  }
  return CMGPU_OK;
}
