// Stand-alone run of hostemu_bai.cpp (the BAM indexer of chromap_amd/csrc/cm_bai.h on the host) for a sanitizer build -- the byte-wise
// loads of records that begin at any offset and end where the allocation ends, the neighbour reads at the first and the last
// record, the windows' and chunks' arrays:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-strict-aliasing
//       tests/hostemu/bai_san_main.cpp -o bai_san && ./bai_san CASE...
// A case file (tests/hostemu_bai_lib.py writes it): the 64-bit words n, n_rec, n_ref, n_blocks, base, want_len, then the n_rec + 1
// starts (64 bits each), the blocks' sizes (32 bits each), the n bytes of records and the want_len bytes the index must be.
// tests/test_hostemu_bai.py builds and runs it.  Exit status 0: every case's index, in every lane mode, is the wanted one.
#include <stdio.h>

#include "hostemu_bai.cpp"

static bool read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) { printf("bai: cannot read %s\n", argv[a]); return 2; }
    uint64_t h[6];
    if (!read_all(f, h, sizeof h)) { printf("bai: %s is no case file\n", argv[a]); return 2; }
    const uint64_t n = h[0], n_rec = h[1], n_ref = h[2], n_blocks = h[3], base = h[4], want_len = h[5];
    std::vector<uint64_t> starts(n_rec + 1);
    std::vector<uint32_t> sizes(n_blocks + 1);
    std::vector<uint8_t> bytes(n + 1), want(want_len + 1), got(want_len + 64);
    if (!read_all(f, starts.data(), (n_rec + 1) * 8) || !read_all(f, sizes.data(), n_blocks * 4) || !read_all(f, bytes.data(), n) || !read_all(f, want.data(), want_len)) {
      printf("bai: %s is cut short\n", argv[a]);
      return 2;
    }
    fclose(f);
    for (int mode = 0; mode < 4; ++mode) {
      uint64_t word = 0;
      const long r = hostemu_bai(bytes.data(), n, starts.data(), n_rec, (uint32_t)n_ref, sizes.data(), n_blocks, base, got.data(), got.size(), mode, &word);
      if (r != (long)want_len || memcmp(got.data(), want.data(), want_len)) {
        printf("bai: %s, mode %d: %ld bytes, want %llu, or other bytes\n", argv[a], mode, r, (unsigned long long)want_len);
        return 1;
      }
    }
    printf("bai: %s: %llu records, %llu bytes of index, four modes equal\n", argv[a], (unsigned long long)n_rec, (unsigned long long)want_len);
  }
  return 0;
}
