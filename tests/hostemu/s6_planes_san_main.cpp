// Stand-alone run of the cases of tests/test_s6_planes_cpu.py (hostemu_s6_planes.cpp: cm_hamming_diag_planes against cm_hamming_diag,
// cm_ref_start_end with the planes arm on and off) for a sanitizer build -- the funnel shifts at g & 31 = 0 and 31, the 64-bit mask at
// L = 64, the third reference record, the bytes the byte form reads past its strings:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-strict-aliasing
//       tests/hostemu/s6_planes_san_main.cpp -o s6_planes_san && ./s6_planes_san
// tests/test_s6_planes_cpu.py builds and runs it.  Exit status 0: every case equal.
#include <stdio.h>

#include "hostemu_s6_planes.cpp"

int main() {
  int32_t bad[6] = {0, 0, 0, 0, 0, 0};
  long total = 0;
  for (uint64_t seed = 1; seed <= 3; ++seed) {
    const long n = hostemu_s6p_sweep(seed, bad);
    if (n < 0) {
      printf("s6_planes: sweep %ld differs at %d %d %d %d %d %d (seed %llu)\n", n, bad[0], bad[1], bad[2], bad[3], bad[4], bad[5], (unsigned long long)seed);
      return 1;
    }
    total += n;
  }
  printf("s6_planes: all %ld cases equal\n", total);
  return 0;
}
