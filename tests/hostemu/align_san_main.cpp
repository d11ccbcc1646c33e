// Stand-alone driver for a sanitizer build of the batch alignment exports of hostemu.cpp (not loaded into Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-strict-aliasing -pthread \
//       tests/hostemu/align_san_main.cpp tests/hostemu/hostemu.cpp chromap_amd/csrc/cm_host.cpp -o align_san && ./align_san
// Gap-rich (window, text) cases for every word-boundary read length and e in {1, 2, 4, 8, 12, 15}, both strands, byte and
// plane forms, the four drop-off shapes, the affine aligner.  Prints the number of cases and a checksum of the results.
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" {
void hostemu_band_batch(int e, int L, uint32_t n, uint32_t off0, const uint8_t *windows, const uint8_t *texts, int strand, int planes,
                        int32_t *err_out, int32_t *end_out);
void hostemu_traceback_batch(int e, int L, uint32_t n, uint32_t off0, const uint8_t *windows, const uint8_t *texts, int strand,
                             const int32_t *errs, int32_t *start_out);
void hostemu_dropoff_batch(int e, int L, uint32_t n, uint32_t off0, const uint8_t *windows, const uint8_t *texts, int shape, int planes,
                           int32_t *err_out, int32_t *end_out, int32_t *len_out);
void hostemu_ksw_batch(int e, int L, uint32_t n, uint32_t off0, const uint8_t *windows, const uint8_t *texts, int strand,
                       int32_t *score_out, int32_t *start_out, int32_t *end_out, uint32_t *cigar_out, int32_t *ncigar_out);
}

int main() {
  uint64_t st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
  const int lens[] = {1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 150}, es[] = {1, 2, 4, 8, 12, 15};
  const uint32_t n = 40;
  uint64_t sum = 0, cases = 0;
  for (int e : es) for (int L : lens) for (int strand = 0; strand < 2; ++strand) {
    const int wl = L + 2 * e;
    std::vector<uint8_t> W((size_t)n * wl), T((size_t)n * L);
    for (uint32_t c = 0; c < n; ++c) {
      uint8_t *w = W.data() + (size_t)c * wl, *t = T.data() + (size_t)c * L;
      for (int i = 0; i < wl; ++i) w[i] = (uint8_t)"ACGTACGTACGTACGTACGTNacgtR"[rnd() % 26];
      int src = e, budget = (int)(rnd() % (uint64_t)(e + 4));
      for (int i = 0; i < L; ++i) {
        if (budget && rnd() % (uint64_t)(L < 8 ? 2 : L / 4) == 0) {
          --budget;
          const int kind = (int)(rnd() % 3), len = 1 + (int)(rnd() % (uint64_t)e);
          if (kind == 0) src += len;
          else if (kind == 1) { for (int k = 0; k < len && i < L; ++k) t[i++] = (uint8_t)"ACGT"[rnd() % 4]; if (i >= L) break; }
          else { t[i] = (uint8_t)"ACGTN"[rnd() % 5]; ++src; continue; }
        }
        t[i] = src < wl ? w[src] : (uint8_t)'A';
        if (strand && !(t[i] == 'A' || t[i] == 'C' || t[i] == 'G' || t[i] == 'T')) t[i] = 'N';
        ++src;
      }
    }
    std::vector<int32_t> a(n), b(n), c3(n), d(n);
    std::vector<uint32_t> cg((size_t)n * 64);
    for (int planes = 0; planes < 2; ++planes) {
      hostemu_band_batch(e, L, n, (uint32_t)L, W.data(), T.data(), strand, planes, a.data(), b.data());
      for (uint32_t c = 0; c < n; ++c) sum += (uint64_t)(uint32_t)a[c] * 31 + (uint32_t)b[c];
    }
    for (uint32_t c = 0; c < n; ++c) if (a[c] > e) a[c] = e;
    hostemu_traceback_batch(e, L, n, (uint32_t)L, W.data(), T.data(), strand, a.data(), b.data());
    for (uint32_t c = 0; c < n; ++c) sum += (uint32_t)b[c];
    if (L >= 25 && 20 - e + 2 < L)
      for (int planes = 0; planes < 2; ++planes) for (int sh = 2 * strand; sh < 2 * strand + 2; ++sh) {
        hostemu_dropoff_batch(e, L, n, (uint32_t)L, W.data(), T.data(), sh, planes, a.data(), b.data(), c3.data());
        for (uint32_t c = 0; c < n; ++c) sum += (uint32_t)a[c] + (uint32_t)b[c] + (uint32_t)c3[c];
      }
    hostemu_ksw_batch(e, L, n, (uint32_t)L, W.data(), T.data(), strand, a.data(), b.data(), c3.data(), cg.data(), d.data());
    for (uint32_t c = 0; c < n; ++c) sum += (uint32_t)a[c] + (uint32_t)d[c];
    cases += n;
  }
  printf("%llu cases, checksum %llu\n", (unsigned long long)cases, (unsigned long long)sum);
  return 0;
}
