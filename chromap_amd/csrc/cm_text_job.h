// cm_text_job.h -- what the device-side text writers share (cm_post.hip: BED / TagAlign, pairs; cm_sam_post.hip: SAM).
// A writer is a sequence of
//   validate -> begin -> (key kernel, sort_pass) x k -> length / select kernel(s) -> scan_lines -> alloc_text -> format kernel -> publish
// with release_sort wherever the writer can spare the sort's buffers.  Every temporary is a CmTmpBuf of the job (or of the writer): a
// return at any point releases what is allocated.
#ifndef CM_TEXT_JOB_H_
#define CM_TEXT_JOB_H_
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <string>
#include <utility>
#include <vector>

#include "cm_barcode_translate.h"
#include "cm_ctx.h"
#include "cm_summary.h"

__device__ __forceinline__ uint32_t cm_digits10(uint32_t v) {
  return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : v < 10000000 ? 7
       : v < 100000000 ? 8 : v < 1000000000 ? 9 : 10;
}
__device__ __forceinline__ uint8_t *cm_put_u32(uint8_t *p, uint32_t v) {
  const uint32_t d = cm_digits10(v);
  for (uint32_t i = d; i-- > 0;) { p[i] = (uint8_t)('0' + v % 10); v /= 10; }
  return p + d;
}

// the context's barcode translation table as the kernels take it (cm_api.hip: cmgpu_set_barcode_translation); none: tab == nullptr
static inline CmBtDev cm_bt_dev(const cmgpu_ctx *c) {
  CmBtDev t;
  t.tab = c->bt_entries ? (const uint64_t *)c->bt_tab.p : nullptr;
  t.blob = (const uint8_t *)c->bt_blob.p;
  t.mask = c->bt_mask;
  t.from_len = c->bt_from;
  return t;
}
// the message of a barcode the table does not have: the reference's own (barcode_translator.h:87)
#define CM_BT_MISS_MESSAGE "Barcode does not exist in the translation table."

struct CmLinesOp {  // a line length -> 1 line, or none
  __host__ __device__ uint64_t operator()(uint64_t l) const { return l ? 1 : 0; }
};

// exclusive scan of n_plus_1 64-bit values on s.  tmp (a DevBuf or a CmTmpBuf) is grown to the scan's work area, and to tmp_also bytes
// for whatever the caller runs on it next.  what: the caller's name for the step in the error message
template <class Buf>
static inline int cm_scan_u64(cmgpu_ctx *c, const uint64_t *in, uint64_t *out, size_t n_plus_1, Buf &tmp, hipStream_t s, const char *what,
                              size_t tmp_also = 0) {
  size_t tb = 0;
  (void)rocprim::exclusive_scan(nullptr, tb, in, out, (uint64_t)0, n_plus_1, rocprim::plus<uint64_t>(), s);
  if (tmp.ensure((tb > tmp_also ? tb : tmp_also) + 256)) { cm_set_error(c, std::string("out of device memory (") + what + ")"); return CMGPU_ENOMEM; }
  const hipError_t e = rocprim::exclusive_scan(tmp.p, tb, in, out, (uint64_t)0, n_plus_1, rocprim::plus<uint64_t>(), s);
  if (e != hipSuccess) { cm_set_error(c, std::string(what) + ": " + hipGetErrorString(e)); return CMGPU_EHIP; }
  return CMGPU_OK;
}

struct CmTextJob {
  cmgpu_ctx *c = nullptr;
  hipStream_t s = nullptr;
  uint32_t n = 0;         // records
  unsigned rid_bits = 1;  // bits of a sort key that hold a sequence id (or one of the rid_extra values past the last)
  std::string blob;       // the uploads' host side: alive until the job ends
  std::vector<uint32_t> noff;
  CmTmpBuf names, name_off;        // the sequence names back to back, their n_sequences + 1 offsets
  CmTmpBuf k0, k1, v0, v1, tmp;    // sort: keys in / out, index in / out, work area (the scan's and the reduction's too)
  CmTmpBuf llen, loff, count;      // n + 1 line lengths, their offsets; four 64-bit words: lines, and three for the writer
  uint64_t *ka = nullptr, *kb = nullptr;
  uint32_t *va = nullptr, *vb = nullptr;

  int enomem(const char *what) { cm_set_error(c, std::string("out of device memory (") + what + ")"); return CMGPU_ENOMEM; }

  // names -> device, key and index arrays (lengths_now: and the line arrays, before anything is uploaded), rid_bits for
  // n_sequences + rid_extra values
  int begin(cmgpu_ctx *ctx, const char *const *seq_names, uint32_t n_sequences, uint32_t n_records, unsigned rid_extra, bool lengths_now) {
    c = ctx; s = ctx->stream; n = n_records;
    noff.assign((size_t)n_sequences + 1, 0);
    for (uint32_t i = 0; i < n_sequences; ++i) { blob += seq_names[i]; noff[i + 1] = (uint32_t)blob.size(); }
    if (names.ensure(blob.size() + 16) || name_off.ensure(noff.size() * 4) || k0.ensure((size_t)n * 8) || k1.ensure((size_t)n * 8) ||
        v0.ensure((size_t)n * 4) || v1.ensure((size_t)n * 4)) return enomem("post-processing");
    if (lengths_now) { const int rc = alloc_lengths(); if (rc) return rc; }
    if (hipMemcpyAsync(names.p, blob.data(), blob.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(name_off.p, noff.data(), noff.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) { cm_set_error(c, "name upload failed"); return CMGPU_EHIP; }
    ka = (uint64_t *)k0.p; kb = (uint64_t *)k1.p;
    va = (uint32_t *)v0.p; vb = (uint32_t *)v1.p;
    while (rid_bits < 32 && (1ull << rid_bits) < (uint64_t)n_sequences + rid_extra) ++rid_bits;
    return CMGPU_OK;
  }
  // the line arrays and the four count words (a writer that frees the sort's buffers before its selection asks for them only then)
  int alloc_lengths() {
    return llen.ensure(((size_t)n + 1) * 8) || loff.ensure(((size_t)n + 1) * 8) || count.ensure(32) ? enomem("post-processing") : CMGPU_OK;
  }
  // the second to fourth count words are the writer's: zero_counts before its kernels count in extra_word()[0] .. [2], scan_lines
  // brings the values back
  unsigned long long *extra_word() const { return (unsigned long long *)count.p + 1; }
  int zero_counts() {
    if (hipMemsetAsync(count.p, 0, 32, s) != hipSuccess) { cm_set_error(c, "memset failed"); return CMGPU_EHIP; }
    return CMGPU_OK;
  }

  uint64_t *keys() const { return ka; }  // where the writer's key kernel writes the next pass's keys
  uint32_t *idx() const { return va; }   // the records' order so far
  const uint32_t *seq_off() const { return (const uint32_t *)name_off.p; }
  // one stable radix pass over the low `bits` bits of keys(), carrying idx()
  int sort_pass(unsigned bits) {
    size_t tb = 0;
    CM_HIPCHECK(c, rocprim::radix_sort_pairs(nullptr, tb, ka, kb, va, vb, (size_t)n, 0, bits, s));
    if (tmp.ensure(tb + 256)) return enomem("sort");
    CM_HIPCHECK(c, rocprim::radix_sort_pairs(tmp.p, tb, ka, kb, va, vb, (size_t)n, 0, bits, s));
    std::swap(va, vb);
    return CMGPU_OK;
  }
  // keys, the spare index array and the work area go; idx() stays
  void release_sort() {
    tmp.release(); k0.release(); k1.release();
    (va == (uint32_t *)v0.p ? v1 : v0).release();
  }

  // line lengths -> offsets, bytes and lines of the text; waits for the stream, after which the count words are released.
  // word1 .. word3: receive the second to fourth count words (extra_word)
  int scan_lines(uint64_t *total, uint64_t *lines, uint64_t *word1 = nullptr, uint64_t *word2 = nullptr, uint64_t *word3 = nullptr) {
    const uint64_t *len = (const uint64_t *)llen.p;
    if (hipMemsetAsync((uint64_t *)llen.p + n, 0, 8, s) != hipSuccess) { cm_set_error(c, "memset failed"); return CMGPU_EHIP; }
    size_t tb2 = 0;
    auto lines_in = rocprim::make_transform_iterator(len, CmLinesOp());
    (void)rocprim::reduce(nullptr, tb2, lines_in, (uint64_t *)nullptr, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s);
    { const int rc = cm_scan_u64(c, len, (uint64_t *)loff.p, (size_t)n + 1, tmp, s, "post-processing scan", tb2); if (rc) return rc; }
    hipError_t e = rocprim::reduce(tmp.p, tb2, lines_in, (uint64_t *)count.p, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s);
    if (e == hipSuccess) e = hipMemcpyAsync(total, (uint64_t *)loff.p + n, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(lines, count.p, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && word1) e = hipMemcpyAsync(word1, (uint64_t *)count.p + 1, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && word2) e = hipMemcpyAsync(word2, (uint64_t *)count.p + 2, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && word3) e = hipMemcpyAsync(word3, (uint64_t *)count.p + 3, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = cm_stream_sync(s);
    count.release();
    if (e != hipSuccess) { cm_set_error(c, std::string("post-processing scan: ") + hipGetErrorString(e)); return CMGPU_EHIP; }
    return cm_summary_check(c);
  }
  int alloc_text(uint64_t total, const std::string &what = "text") { return c->text.ensure(total + 64) ? enomem(what.c_str()) : CMGPU_OK; }
  // after the format kernel: waits for it, then the text is the context's
  int publish(uint64_t total, uint64_t lines, uint64_t *n_lines, uint64_t *n_bytes) {
    const hipError_t e = cm_stream_sync(s);
    if (e != hipSuccess) { cm_set_error(c, std::string("text formatting: ") + hipGetErrorString(e)); return CMGPU_EHIP; }
    c->text_bytes = total;
    ++c->text_gen;
    c->text_lines = lines;
    c->text_bam = false;  // (cmgpu_store_format_bam sets it behind this call)
    *n_lines = lines;
    *n_bytes = total;
    return CMGPU_OK;
  }
};
#endif
