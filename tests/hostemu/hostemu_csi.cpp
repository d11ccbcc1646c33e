// hostemu_csi.cpp -- TEST INFRASTRUCTURE.  The device's CSI indexer (chromap_amd/csrc/cm_tabix.h, cm_bai.h, cm_tabix.hip) on the host,
// both flavours: the same per-record, per-line and per-chunk functions with the depth in their arrays, the same loffset function per
// merged chunk and the same serialiser, run by plain loops in place of the kernels, std::stable_sort in place of the radix sort and
// sequential scans.  The loops' orders are hostemu_bai.cpp's (its `each`, its waves for the records' flags): mode 0 ascending, 1 waves
// of 64, 2 descending, 3 blocks of 256 with the last block first -- what they leave must not depend on who comes first.  The tiles of
// the text's line search, which the depth does not touch, run with one lane.  The bytes lie in a buffer of exactly their size, the
// per-item arrays between guard words, the windows with two spare words that must stay all ones.
#include "hostemu_bai.cpp"

namespace {
struct OneLane {
  static constexpr int G = 1;
  uint32_t t = 0;
  uint32_t scan(uint32_t v, uint32_t *total) { *total = v; return 0; }
  uint32_t sum(uint32_t v) { return v; }
};
struct Guarded {  // n words between two runs of guard words
  static constexpr uint32_t GUARD = 0xA5A5A5A5u;
  static constexpr size_t W = 8;
  std::vector<uint32_t> room;
  size_t n;
  explicit Guarded(size_t n_) : room(n_ + 2 * W, GUARD), n(n_) {}
  uint32_t *p() { return room.data() + W; }
  bool ok() const {
    for (size_t i = 0; i < W; ++i)
      if (room[i] != GUARD || room[W + n + i] != GUARD) return false;
    return true;
  }
};
// stages 3 and 4c, from the raw chunks on: what tx_merge_chunks and k_csi_loffset do
struct Merged {
  std::vector<CmTbxChunk> ch;
  std::vector<uint64_t> loff;
};
void merge(uint32_t depth, const std::vector<uint64_t> &ckey, const std::vector<uint32_t> &cval, const std::vector<uint64_t> &cbeg, const std::vector<uint64_t> &cend,
           const unsigned long long *lin, const uint64_t *lin_off, int mode, Merged &m) {
  const uint32_t n_raw = (uint32_t)ckey.size();
  if (!n_raw) return;
  std::vector<uint64_t> skey(n_raw);
  std::vector<uint32_t> perm = cval, mflag(n_raw);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return ckey[a] < ckey[b]; });
  for (uint32_t j = 0; j < n_raw; ++j) skey[j] = ckey[perm[j]];
  each(n_raw, mode, [&](uint64_t j) { mflag[j] = cm_tbx_chunk_flag(skey.data(), perm.data(), cbeg.data(), cend.data(), j); });
  inclusive_scan(mflag.data(), n_raw);
  const uint32_t n_merged = mflag[n_raw - 1];
  m.ch.resize(n_merged);
  m.loff.assign(n_merged, 0);
  each(n_raw, mode, [&](uint64_t j) { cm_tbx_chunk_emit(skey.data(), perm.data(), cbeg.data(), cend.data(), mflag.data(), n_raw, j, m.ch.data()); });
  each(n_merged, mode, [&](uint64_t j) {
    m.loff[j] = j == 0 || m.ch[j - 1].key != m.ch[j].key ? cm_csi_bin_loffset(m.ch[j].key, depth, lin, lin_off) : 0ull;
  });
}
void back_fill(std::vector<unsigned long long> &lin, uint64_t n_win) {
  for (uint64_t w = n_win; w-- > 1;)  // (the device's back-fill: one reverse minimum scan over all references' windows)
    if (lin[w] < lin[w - 1]) lin[w - 1] = lin[w];
}
long finish(const std::vector<uint8_t> &payload, uint8_t *out, uint64_t cap) {
  if (payload.size() > cap) return -1;
  memcpy(out, payload.data(), payload.size());
  return (long)payload.size();
}
}  // namespace

// The BAM flavour: hostemu_bai's arguments and results, and the depth (1 .. 6)
extern "C" long hostemu_csi_bam(const uint8_t *bytes_in, uint64_t n, const uint64_t *starts_in, uint64_t n_rec, uint32_t n_ref, const uint32_t *sizes, uint64_t n_blocks,
                                uint64_t base, uint32_t depth, uint8_t *out, uint64_t cap, int mode, uint64_t *err_word) {
  std::vector<uint8_t> payload;
  *err_word = CM_TBX_NO_ERROR;
  std::vector<CmBaiRef> ref(n_ref);
  if (n_ref) memset(ref.data(), 0, n_ref * sizeof(CmBaiRef));
  std::vector<CmCsiRef> cref(n_ref);
  Merged m;
  auto serialize = [&]() {
    for (uint32_t r = 0; r < n_ref; ++r) cref[r] = CmCsiRef{ref[r].vbeg, ref[r].vend, ref[r].n_mapped, ref[r].n_unmapped, ref[r].n_intv ? 1u : 0u, 0u};
    cm_csi_serialize(depth, nullptr, 0, cref.data(), n_ref, m.ch.data(), m.ch.size(), m.loff.data(), payload);
    return finish(payload, out, cap);
  };
  if (n_rec == 0) return serialize();
  const size_t shift = mode == 2 ? 1 : 0;
  uint8_t *room = static_cast<uint8_t *>(malloc(n + shift));  // (malloc, not a vector: the records' n bytes end where the allocation ends)
  if (!room) return -5;
  struct Free { uint8_t *p; ~Free() { free(p); } } free_room{room};
  uint8_t *bytes = room + shift;
  memcpy(bytes, bytes_in, n);
  std::vector<uint64_t> starts(starts_in, starts_in + n_rec + 1), coff(n_blocks + 1, 0), lin_off((size_t)n_ref + 1, 0);
  for (uint64_t k = 0; k < n_blocks; ++k) coff[k + 1] = coff[k] + sizes[k];
  Guarded beg(n_rec), end(n_rec), tid(n_rec), cidx(n_rec);
  unsigned long long err = CM_TBX_NO_ERROR;
  CmBaiArrays d = {};
  d.csi_depth = depth;
  d.t.p = bytes;
  d.t.n = n;
  d.t.n_blocks = n_blocks;
  d.t.coff = coff.data();
  d.t.base = base;
  d.n_rec = n_rec;
  d.starts = starts.data();
  d.n_ref = n_ref;
  d.beg = beg.p();
  d.end = end.p();
  d.tid = tid.p();
  d.cidx = cidx.p();
  d.err = &err;
  d.ref = ref.data();
  each(n_rec, mode, [&](uint64_t i) { cm_bai_rec_parse<HostAtomics>(d, i); });
  if (err != CM_TBX_NO_ERROR) { *err_word = err; return -2; }
  flags(d, mode);
  inclusive_scan(d.cidx, n_rec);
  const uint32_t n_raw = d.cidx[n_rec - 1];
  for (uint32_t r = 0; r < n_ref; ++r) lin_off[r + 1] = lin_off[r] + ref[r].n_intv;
  const uint64_t n_win = lin_off[n_ref];
  std::vector<unsigned long long> lin(n_win + 2, ~0ull);
  std::vector<uint64_t> ckey(n_raw), cbeg(n_raw), cend(n_raw);
  std::vector<uint32_t> cval(n_raw);
  d.lin_off = lin_off.data();
  d.lin = lin.data();
  d.ckey = ckey.data();
  d.cbeg = cbeg.data();
  d.cend = cend.data();
  d.cval = cval.data();
  each(n_rec, mode, [&](uint64_t i) { cm_bai_rec_emit<HostAtomics>(d, i); });
  if (lin[n_win] != ~0ull || lin[n_win + 1] != ~0ull) return -4;
  if (!beg.ok() || !end.ok() || !tid.ok() || !cidx.ok()) return -4;
  back_fill(lin, n_win);
  merge(depth, ckey, cval, cbeg, cend, lin.data(), lin_off.data(), mode, m);
  return serialize();
}

// The tabix flavour: the text's n bytes and its blocks' sizes, as hostemu_tabix takes them.  -3: no final newline
extern "C" long hostemu_csi_bed(const uint8_t *text_in, uint64_t n, const uint32_t *sizes, uint64_t n_blocks, uint64_t base, uint32_t depth, uint8_t *out, uint64_t cap,
                                int mode, uint64_t *err_word) {
  std::vector<uint8_t> payload, aux;
  *err_word = CM_TBX_NO_ERROR;
  if (n == 0) {
    cm_csi_tabix_aux(0, nullptr, nullptr, aux);
    cm_csi_serialize(depth, aux.data(), (uint32_t)aux.size(), nullptr, 0, nullptr, 0, nullptr, payload);
    return finish(payload, out, cap);
  }
  const size_t shift = mode == 2 ? 1 : 0;
  uint8_t *room = static_cast<uint8_t *>(malloc(n + shift));
  if (!room) return -5;
  struct Free { uint8_t *p; ~Free() { free(p); } } free_room{room};
  uint8_t *text = room + shift;
  memcpy(text, text_in, n);
  std::vector<uint64_t> coff(n_blocks + 1, 0);
  for (uint64_t k = 0; k < n_blocks; ++k) coff[k + 1] = coff[k] + sizes[k];
  CmTbxArrays d = {};
  d.csi_depth = depth;
  d.t.p = text;
  d.t.n = n;
  d.t.n_blocks = n_blocks;
  d.t.coff = coff.data();
  d.t.base = base;
  // 1. line starts (one lane)
  const uint64_t n_tiles = (n + CM_TBX_TILE - 1) / CM_TBX_TILE;
  std::vector<uint64_t> toff(n_tiles + 1, 0);
  OneLane g;
  for (uint64_t t = 0; t < n_tiles; ++t) toff[t + 1] = toff[t] + cm_tbx_tile_count(g, text, n, t);
  const uint64_t n_lines = toff[n_tiles];
  if (text[n - 1] != '\n') return -3;
  std::vector<uint64_t> lstart(n_lines + 1, 0);
  for (uint64_t t = 0; t < n_tiles; ++t) cm_tbx_tile_starts(g, text, n, t, toff[t], lstart.data());
  if (lstart[n_lines] != n) return -4;
  // 2. per line
  Guarded beg(n_lines), end(n_lines), tid(n_lines), cidx(n_lines);
  unsigned long long err = CM_TBX_NO_ERROR;
  d.n_lines = n_lines;
  d.lstart = lstart.data();
  d.beg = beg.p();
  d.end = end.p();
  d.tid = tid.p();
  d.cidx = cidx.p();
  d.err = &err;
  each(n_lines, mode, [&](uint64_t i) { cm_tbx_line_parse<HostAtomics>(d, i); });
  inclusive_scan(d.tid, n_lines);
  if (err != CM_TBX_NO_ERROR) { *err_word = err; return -2; }
  const uint32_t n_ref = d.tid[n_lines - 1];
  std::vector<CmTbxRef> ref(n_ref);
  memset(ref.data(), 0, n_ref * sizeof(CmTbxRef));
  d.ref = ref.data();
  each(n_lines, mode, [&](uint64_t i) {
    uint32_t t;
    unsigned long long e = CM_TBX_NO_ERROR;
    const uint32_t want = cm_tbx_line_flags_core(d, i, &t, &e);
    HostAtomics::min64(&err, e);
    if (want > ref[t].n_intv) ref[t].n_intv = want;
  });
  inclusive_scan(d.cidx, n_lines);
  if (err != CM_TBX_NO_ERROR) { *err_word = err; return -2; }
  const uint32_t n_raw = d.cidx[n_lines - 1];
  std::vector<uint64_t> name_off((size_t)n_ref + 1, 0), lin_off((size_t)n_ref + 1, 0);
  for (uint32_t r = 0; r < n_ref; ++r) {
    name_off[r + 1] = name_off[r] + ref[r].name_len;
    lin_off[r + 1] = lin_off[r] + ref[r].n_intv;
  }
  std::vector<uint8_t> names(name_off[n_ref] + 1);
  for (uint32_t r = 0; r < n_ref; ++r) memcpy(names.data() + name_off[r], text + ref[r].name_at, ref[r].name_len);
  for (uint32_t r = 0; r < n_ref; ++r)  // (a plain search: the test texts have few names)
    for (uint32_t q = 0; q < r; ++q)
      if (ref[q].name_len == ref[r].name_len && !memcmp(names.data() + name_off[q], names.data() + name_off[r], ref[r].name_len)) {
        *err_word = (uint64_t)ref[r].first_line << 3 | CM_TBX_E_RECUR;
        return -2;
      }
  const uint64_t n_win = lin_off[n_ref];
  std::vector<unsigned long long> lin(n_win + 2, ~0ull);
  std::vector<uint64_t> ckey(n_raw), cbeg(n_raw), cend(n_raw);
  std::vector<uint32_t> cval(n_raw);
  d.lin_off = lin_off.data();
  d.lin = lin.data();
  d.ckey = ckey.data();
  d.cbeg = cbeg.data();
  d.cend = cend.data();
  d.cval = cval.data();
  each(n_lines, mode, [&](uint64_t i) { cm_tbx_line_emit<HostAtomics>(d, i); });
  if (lin[n_win] != ~0ull || lin[n_win + 1] != ~0ull) return -4;
  if (!beg.ok() || !end.ok() || !tid.ok() || !cidx.ok()) return -4;
  back_fill(lin, n_win);
  // 3. raw chunks, the bins' loffsets; 4c. the payload
  Merged m;
  merge(depth, ckey, cval, cbeg, cend, lin.data(), lin_off.data(), mode, m);
  std::vector<CmCsiRef> cref(n_ref);
  for (uint32_t r = 0; r < n_ref; ++r)
    cref[r] = CmCsiRef{ref[r].vbeg, ref[r].vend, (r + 1 < n_ref ? ref[r + 1].first_line : n_lines) - ref[r].first_line, 0, 1u, 0u};
  cm_csi_tabix_aux(n_ref, names.data(), name_off.data(), aux);
  cm_csi_serialize(depth, aux.data(), (uint32_t)aux.size(), cref.data(), n_ref, m.ch.data(), m.ch.size(), m.loff.data(), payload);
  return finish(payload, out, cap);
}

extern "C" uint32_t hostemu_csi_reg2bin(uint32_t beg, uint32_t end, uint32_t depth) { return cm_csi_reg2bin(beg, end, depth); }
extern "C" uint64_t hostemu_csi_bin_window(uint32_t bin, uint32_t depth) { return cm_csi_bin_window(bin, depth); }
