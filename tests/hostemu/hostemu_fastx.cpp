// hostemu_fastx.cpp -- the record chain of layout CMGPU_FASTX_FREE (chromap_amd/csrc/cm_fastx.h) compiled for the host: the same line
// classes, record walk, tile resolution and concatenating copy as the k_fx_* kernels of cm_ingest.hip, driven by plain loops in the order
// the device launches them.  Test infrastructure only (tests/test_hostemu_fastx.py builds it, also with a tile of a few lines so that
// records straddle every tile boundary).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../chromap_amd/csrc/cm_fastx.h"

extern "C" {

// status of hostemu_fastx_scan
enum { FXE_OK = 0, FXE_TRUNC = 1, FXE_JUNK = 2, FXE_KEPT_CR = 3, FXE_NEEDS_QUAL = 4, FXE_MIXED = 5 };

struct FxScan {
  std::vector<uint32_t> nl, li, nxt, send, sl, recidx;
  std::vector<uint8_t> text;
  uint32_t n_lines = 0, stop = 0, seen = 0;  // seen: CM_FX_SEEN_* over the chunks of one text (CmFqStream::fx_seen)
  bool final_chunk = false;
};

void *hostemu_fastx_new() { return new FxScan(); }
void hostemu_fastx_free(void *p) { delete static_cast<FxScan *>(p); }
uint32_t hostemu_fastx_tile() { return CM_FX_TILE; }

// cmgpu_fastq_scan's general path: the countable records of the chunk; *err_line: the record (or line) a refusal is about
int hostemu_fastx_scan(void *p, const uint8_t *text, uint64_t n, int final_chunk, int want_qual, uint32_t *n_records, uint32_t *err_line) {
  FxScan &f = *static_cast<FxScan *>(p);
  f.text.assign(text, text + n);
  f.nl.clear();
  for (uint64_t i = 0; i < n; ++i) if (text[i] == '\n') f.nl.push_back((uint32_t)i);
  const bool unterminated = final_chunk && n && text[n - 1] != '\n';
  if (unterminated) f.nl.push_back((uint32_t)n);
  const uint32_t n_lines = (uint32_t)f.nl.size();
  f.n_lines = n_lines;
  f.stop = 0;
  f.final_chunk = final_chunk != 0;
  f.recidx.clear();
  *n_records = 0;
  *err_line = CM_FX_NONE;
  if (n_lines == 0) return FXE_OK;
  f.li.resize(n_lines); f.nxt.resize(n_lines); f.send.resize(n_lines); f.sl.resize(n_lines);
  for (uint32_t i = 0; i < n_lines; ++i) f.li[i] = cm_fx_line_info(f.text.data(), f.nl.data(), i);                      // k_fx_lines
  for (uint32_t i = 0; i < n_lines; ++i)                                                                                 // k_fx_walk
    cm_fx_walk(f.li.data(), n_lines, i, final_chunk != 0, unterminated, &f.nxt[i], &f.send[i], &f.sl[i]);
  const uint32_t n_tiles = (n_lines + CM_FX_TILE - 1) / CM_FX_TILE;
  std::vector<uint32_t> exit_(n_lines), entry(n_tiles, CM_FX_NONE), e(CM_FX_TILE);
  for (uint32_t t = 0; t < n_tiles; ++t) {                                                                               // k_fx_tile
    const uint32_t t0 = t * CM_FX_TILE, t1 = t0 + CM_FX_TILE < n_lines ? t0 + CM_FX_TILE : n_lines, cnt = t1 - t0;
    for (uint32_t k = 0; k < cnt; ++k) e[k] = f.nxt[t0 + k];
    for (int r = 0; r < CM_FX_TILE_ROUNDS; ++r)
      for (uint32_t k = 0; k < cnt; ++k) cm_fx_tile_jump(e.data(), t0, t1, k);
    for (uint32_t k = 0; k < cnt; ++k) exit_[t0 + k] = e[k];
  }
  cm_fx_tile_entries(exit_.data(), n_lines, entry.data());                                                               // k_fx_entries
  std::vector<uint8_t> keep(n_lines, 0);
  uint32_t res[4] = {CM_FX_NONE, 0, CM_FX_NONE, 0};
  for (uint32_t t = 0; t < n_tiles; ++t) {                                                                               // k_fx_mark
    if (entry[t] == CM_FX_NONE) continue;
    const uint32_t t1 = (t + 1) * CM_FX_TILE < n_lines ? (t + 1) * CM_FX_TILE : n_lines;
    cm_fx_tile_members(f.nxt.data(), entry[t], t1, [&](uint32_t i) {
      const uint32_t st = f.sl[i] >> 28, len = f.sl[i] & CM_FX_LEN_MASK;
      if (st <= CM_FX_FASTA) {
        if (len == 0) return;
        if (st == CM_FX_FASTA && want_qual) { if (i < res[2]) res[2] = i; }
        else { keep[i] = 1; res[3] |= st == CM_FX_FASTA ? CM_FX_SEEN_FASTA : CM_FX_SEEN_FASTQ; }
      } else if (st != CM_FX_SKIP) { res[0] = i; res[1] = st; }
    });
  }
  for (uint32_t i = 0; i < n_lines; ++i) if (keep[i]) f.recidx.push_back(i);                                             // scan + k_fq_compact
  const bool early = res[0] != CM_FX_NONE, refused = early && res[1] != CM_FX_INCOMPLETE;
  if (res[2] != CM_FX_NONE && !(refused && res[0] < res[2])) { *err_line = res[2]; f.recidx.clear(); return FXE_NEEDS_QUAL; }
  if (refused) {
    *err_line = res[0];
    f.recidx.clear();
    return res[1] == CM_FX_TRUNC ? FXE_TRUNC : res[1] == CM_FX_KEPT_CR ? FXE_KEPT_CR : FXE_JUNK;
  }
  f.seen |= res[3];
  if (f.seen == (CM_FX_SEEN_FASTQ | CM_FX_SEEN_FASTA)) { f.recidx.clear(); return FXE_MIXED; }
  f.stop = early ? res[0] : n_lines;
  *n_records = (uint32_t)f.recidx.size();
  return FXE_OK;
}

// cmgpu_fastq_take's general path for the first n records of the last scan: bases / quals (quals may be null) back to back with n + 1
// offsets, names likewise, has_qual[j], and the byte where the next chunk starts.  --read-format as cmgpu_fastq_set_format.
uint64_t hostemu_fastx_take(void *p, uint32_t n, int n_ranges, const int *starts, const int *ends, int minus, uint8_t *bases, uint8_t *quals,
                            uint32_t *offsets, uint8_t *names, uint32_t *name_offsets, uint8_t *has_qual) {
  FxScan &f = *static_cast<FxScan *>(p);
  const uint8_t *text = f.text.data();
  const uint32_t *nl = f.nl.data();
  const uint64_t n_bytes = f.text.size();
  uint32_t line = f.stop;
  if (f.final_chunk && n == f.recidx.size()) f.seen = 0;
  if (n < f.recidx.size()) line = n ? f.nxt[f.recidx[n - 1]] : 0;
  uint64_t consumed = 0;
  if (line > 0) { consumed = (uint64_t)nl[line - 1] + 1; if (consumed > n_bytes) consumed = n_bytes; }
  offsets[0] = 0;
  name_offsets[0] = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t h = f.recidx[j], raw = f.sl[h] & CM_FX_LEN_MASK;
    uint32_t l = raw;
    if (n_ranges) {  // (fq_eff_len, cm_ingest.hip)
      l = 0;
      for (int k = 0; k < n_ranges; ++k) {
        int st = starts[k], en = ends[k] == -1 ? (int)raw - 1 : ends[k];
        if (en >= (int)raw) en = (int)raw - 1;
        if (st < 0) st = 0;
        if (en >= st) l += (uint32_t)(en - st + 1);
      }
    }
    const uint32_t o = offsets[j];
    offsets[j + 1] = o + l;
    cm_fx_copy(text, nl, h + 1, f.send[h], raw, n_ranges, starts, ends, minus, minus != 0, o, l, bases);
    has_qual[j] = (f.sl[h] >> 28) == CM_FX_FASTQ;
    if (quals) {
      if (has_qual[j]) cm_fx_copy(text, nl, f.send[h] + 1, f.nxt[h], raw, n_ranges, starts, ends, minus, false, o, l, quals);
      else memset(quals + o, 0, l);
    }
    // the name: behind the marker up to the first isspace() byte (k_fq_name_len's rule)
    uint32_t s = (h == 0 ? 0u : nl[h - 1] + 1u) + 1u, e = s;
    while (e < n_bytes && !cm_fx_isspace(text[e])) ++e;
    memcpy(names + name_offsets[j], text + s, e - s);
    name_offsets[j + 1] = name_offsets[j] + (e - s);
  }
  return consumed;
}

}  // extern "C"
