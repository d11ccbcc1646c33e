// Stand-alone run of the MAPQ stage functions (hostemu_mapq_batch, hostemu_valu.cpp) on the case file tests/test_mapq_cpu.py writes,
// for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=undefined -ffp-contract=off
//       -fno-strict-aliasing tests/hostemu/mapq_san_main.cpp -o mapq_san && ./mapq_san CASES
// A clean run shows that the cases stay inside defined behaviour: no double leaves the range of the integer it is converted to, no
// signed overflow, no division by zero, no table read out of bounds.  The file: int64 number of groups; per group int64 kind, e, n,
// then the reads matrix (9 x 2 n int32), the pairs matrix (6 x n int32) and the n bytes of the model (tests/mapq_model.py).
// Exit status 0: every byte equals the model's.
#include <stdio.h>

#include "hostemu_valu.cpp"

static bool get(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: mapq_san CASES\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int64_t n_groups = 0;
  if (!get(f, &n_groups, 8)) { fprintf(stderr, "short file\n"); return 2; }
  uint64_t total = 0;
  for (int64_t g = 0; g < n_groups; ++g) {
    int64_t hdr[3];
    if (!get(f, hdr, sizeof hdr) || hdr[2] < 0 || hdr[2] > (1ll << 30)) { fprintf(stderr, "group %lld: bad header\n", (long long)g); return 2; }
    const size_t n = (size_t)hdr[2];
    std::vector<int32_t> reads(9 * 2 * n), pairs(6 * n);
    std::vector<uint8_t> want(n), got(n, 0xEE);
    if (!get(f, reads.data(), reads.size() * 4) || !get(f, pairs.data(), pairs.size() * 4) || !get(f, want.data(), n)) {
      fprintf(stderr, "group %lld: short file\n", (long long)g);
      return 2;
    }
    if (hostemu_mapq_batch((int)hdr[0], (int)hdr[1], n, reads.data(), pairs.data(), got.data(), nullptr, nullptr, 0, nullptr) != 0) {
      fprintf(stderr, "group %lld: bad arguments\n", (long long)g);
      return 2;
    }
    for (size_t i = 0; i < n; ++i)
      if (got[i] != want[i]) {
        fprintf(stderr, "group %lld (kind %lld, e %lld) case %zu: %u here, %u in the model\n", (long long)g, (long long)hdr[0], (long long)hdr[1], i,
                (unsigned)got[i], (unsigned)want[i]);
        return 1;
      }
    total += n;
  }
  fclose(f);
  printf("mapq: %llu cases equal\n", (unsigned long long)total);
  return 0;
}
