// cm_bgzf_out.hip -- BGZF output compressed on the device (cm_deflate.h): the text store, or any bytes, cut into slices of 0xff00 bytes,
// one BGZF block per slice.  A chunk of BZ_CHUNK slices at a time: k_bgzf_deflate -- a workgroup per slice, BZ_GROUPS workgroups that
// take the chunk's slices in turn -- writes every block into a slot of 64 KiB and its size into a table; the host adds the sizes up and
// makes room in the packed store, k_bgzf_gather moves the blocks there back to back.  Device memory besides the packed blocks: the
// slots (BZ_CHUNK * 64 KiB = 128 MiB), the groups' token arrays (BZ_GROUPS * 0xff00 words = 127.5 MiB) and the sizes (8 KiB), whatever
// the text's length.
// The small texts the host writes itself (header lines) become stored-deflate blocks built on the host; the 28-byte empty block that
// ends a BGZF file is written once, last.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "cm_ctx.h"
#include "cm_deflate.h"

#define BZ_CHUNK 2048u   // slices per launch
#define BZ_GROUPS 512u   // workgroups per launch: two per compute unit
#define BZ_LANES 256

// the group type cm_deflate.h asks for: the workgroup
struct BzGroup {
  static constexpr int G = BZ_LANES;
  static constexpr int W = 64;
  uint32_t t;
  uint32_t *xw;  // G / W words of shared memory: the waves' totals
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ void wsync() {  // the lanes of a wave: their shared-memory writes before it are seen after it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
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
    for (int q = 0; q < G / W; ++q) { const uint32_t x = xw[q]; base += (uint32_t)q < wv ? x : 0u; tot += x; }
    __syncthreads();
    *total = tot;
    return base + incl - v;
  }
  __device__ __forceinline__ uint32_t sum(uint32_t v) { uint32_t tot; (void)scan(v, &tot); return tot; }
};

// slices first .. first + n_slices - 1 of text[0 .. n_bytes): block b of the chunk to slots + b * CM_DF_SLOT, its size to sizes[b]
// (two waves per SIMD: the two workgroups per compute unit that shared memory allows; without the bound the compiler takes 391 registers)
__global__ __launch_bounds__(BZ_LANES, 2) void k_bgzf_deflate(const uint8_t *__restrict__ text, uint64_t n_bytes, uint64_t first, uint32_t n_slices,
                                                          uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes, uint32_t *__restrict__ tok, CmCrcX2n x2n) {
  __shared__ CmDfShared sh;
  __shared__ uint32_t xw[BZ_LANES / 64];
  __shared__ uint32_t x2[32];
  BzGroup g;
  g.t = threadIdx.x;
  g.xw = xw;
  if (g.t < 32) x2[g.t] = x2n.v[g.t];
  __syncthreads();
  for (uint32_t b = blockIdx.x; b < n_slices; b += gridDim.x) {
    const uint64_t off = (first + b) * (uint64_t)CM_DF_SLICE;
    const uint32_t n = n_bytes - off < CM_DF_SLICE ? (uint32_t)(n_bytes - off) : CM_DF_SLICE;
    const uint32_t total = cm_deflate_block(g, text + off, n, slots + (size_t)b * CM_DF_SLOT, tok + (size_t)blockIdx.x * CM_DF_SLICE, sh, x2);
    if (g.t == 0) sizes[b] = total;
  }
}
// block b of the chunk to out + (the sizes of the blocks before it).  coff (the chunk's part of the store's offset table): block b's
// offset in the store -- `used` bytes stand before the chunk -- and behind the chunk's last block the offset of whatever follows
__global__ __launch_bounds__(BZ_LANES) void k_bgzf_gather(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes, uint8_t *__restrict__ out,
                                                       uint64_t *__restrict__ coff, uint64_t used) {
  __shared__ uint32_t before;
  const uint32_t b = blockIdx.x;
  if (threadIdx.x == 0) before = 0;
  __syncthreads();
  uint32_t mine = 0;  // (a chunk's blocks together: less than 2^27 bytes)
  for (uint32_t j = threadIdx.x; j < b; j += BZ_LANES) mine += sizes[j];
  if (mine) atomicAdd(&before, mine);
  __syncthreads();
  const uint8_t *src = slots + (size_t)b * CM_DF_SLOT;
  uint8_t *dst = out + before;
  const uint32_t n = sizes[b];
  if (threadIdx.x == 0) {
    coff[b] = used + before;
    if (b + 1 == gridDim.x) coff[b + 1] = used + before + n;
  }
  // whole words where the destination is aligned (a slot is), the bytes around them one by one
  const uint32_t head = (uint32_t)((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u);
  const uint32_t h = head < n ? head : n;
  if (threadIdx.x < h) dst[threadIdx.x] = src[threadIdx.x];
  const uint32_t nw = (n - h) / 4u;
  uint32_t *dw = reinterpret_cast<uint32_t *>(dst + h);
  for (uint32_t i = threadIdx.x; i < nw; i += BZ_LANES) {
    const uint8_t *s = src + h + 4u * i;
    dw[i] = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
  }
  const uint32_t tail = h + 4u * nw;
  if (tail + threadIdx.x < n) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
}

static const CmCrcX2n &bz_x2n() {
  static const CmCrcX2n x = []() { CmCrcX2n t; cm_crc_x2n_table(t); return t; }();
  return x;
}

// n_bytes of device memory at `text` into the compressed store
// (src: CM_BZ_SRC_*, what `text` is -- the tabix indexer reads the same text again)
static int bz_compress_device(cmgpu_ctx *c, const uint8_t *text, uint64_t n_bytes, int src, uint64_t *n_blocks, uint64_t *n_out) {
  hipStream_t s = c->stream;
  c->bgzf_bytes = 0;
  c->bgzf_blocks = 0;
  c->bgzf_text_bytes = 0;
  c->bgzf_src = CM_BZ_SRC_NONE;
  const uint64_t n_slices = (n_bytes + CM_DF_SLICE - 1) / CM_DF_SLICE;
  if (n_slices) {
    const uint32_t chunk = n_slices < BZ_CHUNK ? (uint32_t)n_slices : BZ_CHUNK;
    const uint32_t groups = chunk < BZ_GROUPS ? chunk : BZ_GROUPS;
    if (c->bgzf_slots.ensure((size_t)chunk * CM_DF_SLOT) || c->bgzf_tok.ensure((size_t)groups * CM_DF_SLICE * 4) || c->bgzf_sizes.ensure((size_t)chunk * 4) ||
        c->bgzf_coff.ensure((size_t)(n_slices + 1) * 8)) {
      cm_set_error(c, "out of device memory (BGZF output: scratch)"); return CMGPU_ENOMEM;
    }
  }
  std::vector<uint32_t> sizes;
  uint64_t used = 0;
  for (uint64_t first = 0; first < n_slices; first += BZ_CHUNK) {
    const uint32_t m = n_slices - first < BZ_CHUNK ? (uint32_t)(n_slices - first) : BZ_CHUNK;
    const uint32_t groups = m < BZ_GROUPS ? m : BZ_GROUPS;
    hipLaunchKernelGGL(k_bgzf_deflate, dim3(groups), dim3(BZ_LANES), 0, s, text, n_bytes, first, m, (uint8_t *)c->bgzf_slots.p, (uint32_t *)c->bgzf_sizes.p,
                       (uint32_t *)c->bgzf_tok.p, bz_x2n());
    CM_HIPCHECK(c, hipGetLastError());  // (a launch that did not happen would leave the sizes of the chunk before)
    sizes.resize(m);
    CM_HIPCHECK(c, hipMemcpyAsync(sizes.data(), c->bgzf_sizes.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    CM_HIPCHECK(c, cm_stream_sync(s));
    uint64_t add = 0;
    for (uint32_t i = 0; i < m; ++i) {
      if (sizes[i] < 28u || sizes[i] >= CM_DF_SLOT) { cm_set_error(c, "BGZF output: a block of impossible size"); return CMGPU_EHIP; }
      add += sizes[i];
    }
    // (the first guess: a third of the text, which SAM and pairs text stay under; then doubling)
    const int rc = cm_grow_buf(c, c->bgzf, used, used + add + 16, n_bytes / 3 + (1u << 20), s, "BGZF output");
    if (rc) return rc;
    hipLaunchKernelGGL(k_bgzf_gather, dim3(m), dim3(BZ_LANES), 0, s, (const uint8_t *)c->bgzf_slots.p, (const uint32_t *)c->bgzf_sizes.p, (uint8_t *)c->bgzf.p + used,
                       (uint64_t *)c->bgzf_coff.p + first, used);
    CM_HIPCHECK(c, hipGetLastError());
    used += add;
  }
  CM_HIPCHECK(c, cm_stream_sync(s));
  c->bgzf_bytes = used;
  c->bgzf_blocks = n_slices;
  c->bgzf_text_bytes = n_bytes;
  c->bgzf_src = src;
  c->bgzf_src_ptr = src == CM_BZ_SRC_DEVICE ? text : nullptr;
  c->bgzf_text_gen = c->text_gen;
  if (n_blocks) *n_blocks = n_slices;
  if (n_out) *n_out = used;
  return CMGPU_OK;
}

extern "C" int cmgpu_bgzf_compress(cmgpu_ctx *c, const void *text, uint64_t n_bytes, int on_device, uint64_t *n_blocks, uint64_t *n_out) {
  if (!c || (!text && n_bytes)) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  const uint8_t *dev = static_cast<const uint8_t *>(text);
  if (!on_device && n_bytes) {
    if (c->bgzf_in.ensure(n_bytes + 16)) { cm_set_error(c, "out of device memory (BGZF output: text)"); return CMGPU_ENOMEM; }
    CM_HIPCHECK(c, hipMemcpyAsync(c->bgzf_in.p, text, n_bytes, hipMemcpyHostToDevice, c->stream));
    dev = static_cast<const uint8_t *>(c->bgzf_in.p);
  }
  return bz_compress_device(c, dev, n_bytes, on_device ? CM_BZ_SRC_DEVICE : CM_BZ_SRC_UPLOAD, n_blocks, n_out);
}
extern "C" int cmgpu_store_compress_text(cmgpu_ctx *c, uint64_t *n_blocks, uint64_t *n_out) {
  if (!c) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  return bz_compress_device(c, static_cast<const uint8_t *>(c->text.p), c->text_bytes, CM_BZ_SRC_STORE, n_blocks, n_out);
}
extern "C" int cmgpu_bgzf_info(const cmgpu_ctx *c, uint64_t *n_blocks, uint64_t *n_bytes, uint64_t *n_text_bytes) {
  if (!c) return CMGPU_EINVAL;
  if (n_blocks) *n_blocks = c->bgzf_blocks;
  if (n_bytes) *n_bytes = c->bgzf_bytes;
  if (n_text_bytes) *n_text_bytes = c->bgzf_text_bytes;
  return CMGPU_OK;
}
extern "C" int cmgpu_bgzf_download(cmgpu_ctx *c, void *out, uint64_t capacity) {
  if (!c || (!out && c->bgzf_bytes)) return CMGPU_EINVAL;
  if (capacity < c->bgzf_bytes) { cm_set_error(c, "BGZF buffer too small"); return CMGPU_ECAPACITY; }
  CM_HIPCHECK(c, cm_enter(c));
  if (c->bgzf_bytes) CM_HIPCHECK(c, hipMemcpy(out, c->bgzf.p, c->bgzf_bytes, hipMemcpyDeviceToHost));
  return CMGPU_OK;
}
extern "C" int cmgpu_bgzf_write(cmgpu_ctx *c, const char *path, int append) {
  if (!c || !path) return CMGPU_EINVAL;
  CM_HIPCHECK(c, cm_enter(c));
  return cm_write_device_bytes(c, c->bgzf.p, c->bgzf_bytes, path, append, "the BGZF blocks");
}

// ---- on the host: stored blocks for the few header lines, and the end-of-file block ----
static uint32_t bz_host_crc(const uint8_t *p, size_t n) {
  static const std::vector<uint32_t> tab = []() { std::vector<uint32_t> t(256); for (uint32_t i = 0; i < 256; ++i) t[i] = cm_crc32_entry(i); return t; }();
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) c = tab[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return c ^ 0xffffffffu;
}
extern "C" int cmgpu_bgzf_write_host_text(const char *path, const void *text, uint64_t n, int append) {
  if (!path || (!text && n)) return CMGPU_EINVAL;
  FILE *f = fopen(path, append ? "ab" : "wb");
  if (!f) return CMGPU_EIO;
  const uint8_t *p = static_cast<const uint8_t *>(text);
  std::vector<uint8_t> blk(CM_DF_SLICE + 31u);
  bool ok = true;
  for (uint64_t off = 0; ok && off < n; off += CM_DF_SLICE) {
    const uint32_t m = n - off < CM_DF_SLICE ? (uint32_t)(n - off) : CM_DF_SLICE;
    const uint32_t total = 18u + 5u + m + 8u;
    cm_df_bgzf_header(blk.data(), total);
    blk[18] = 1;  // the last block of the stream, stored
    blk[19] = (uint8_t)(m & 0xffu);
    blk[20] = (uint8_t)(m >> 8);
    blk[21] = (uint8_t)(~m & 0xffu);
    blk[22] = (uint8_t)((~m >> 8) & 0xffu);
    memcpy(blk.data() + 23, p + off, m);
    cm_df_bgzf_trailer(blk.data() + 23 + m, bz_host_crc(p + off, m), m);
    ok = fwrite(blk.data(), 1, total, f) == total;
  }
  ok = fclose(f) == 0 && ok;
  return ok ? CMGPU_OK : CMGPU_EIO;
}
extern "C" int cmgpu_bgzf_write_eof(const char *path) {
  if (!path) return CMGPU_EINVAL;
  static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  FILE *f = fopen(path, "ab");
  if (!f) return CMGPU_EIO;
  bool ok = fwrite(eof, 1, sizeof eof, f) == sizeof eof;
  ok = fclose(f) == 0 && ok;
  return ok ? CMGPU_OK : CMGPU_EIO;
}
