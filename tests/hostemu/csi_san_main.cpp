// Stand-alone run of hostemu_csi.cpp (the CSI indexer of chromap_amd/csrc/cm_tabix.h and cm_bai.h on the host, both flavours) for a
// sanitizer build -- the 64-bit sums and shifts of positions up to 2^32, the walk from a bin's number to its first window, the
// windows' and chunks' arrays, the byte-wise loads of records and lines that end where the allocation ends:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-strict-aliasing
//       tests/hostemu/csi_san_main.cpp -o csi_san && ./csi_san CASE...
// A case file (tests/hostemu_csi_lib.py writes it): the 64-bit words flavour (0 BAM, 1 tabix), n, n_rec, n_ref, n_blocks, base, depth,
// want_len, then -- BAM flavour only -- the n_rec + 1 starts (64 bits each), the blocks' sizes (32 bits each), the n bytes of records
// or text and the want_len bytes the index must be.  tests/test_hostemu_csi.py builds and runs it.  Exit status 0: every case's
// index, in every lane mode, is the wanted one.
#include <stdio.h>

#include "hostemu_csi.cpp"

static bool read_all(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) { printf("csi: cannot read %s\n", argv[a]); return 2; }
    uint64_t h[8];
    if (!read_all(f, h, sizeof h)) { printf("csi: %s is no case file\n", argv[a]); return 2; }
    const uint64_t flavour = h[0], n = h[1], n_rec = h[2], n_ref = h[3], n_blocks = h[4], base = h[5], depth = h[6], want_len = h[7];
    std::vector<uint64_t> starts(flavour == 0 ? n_rec + 1 : 1);
    std::vector<uint32_t> sizes(n_blocks + 1);
    std::vector<uint8_t> bytes(n + 1), want(want_len + 1), got(want_len + 64);
    if ((flavour == 0 && !read_all(f, starts.data(), (n_rec + 1) * 8)) || !read_all(f, sizes.data(), n_blocks * 4) || !read_all(f, bytes.data(), n) ||
        !read_all(f, want.data(), want_len)) {
      printf("csi: %s is cut short\n", argv[a]);
      return 2;
    }
    fclose(f);
    for (int mode = 0; mode < 4; ++mode) {
      uint64_t word = 0;
      const long r = flavour == 0 ? hostemu_csi_bam(bytes.data(), n, starts.data(), n_rec, (uint32_t)n_ref, sizes.data(), n_blocks, base, (uint32_t)depth, got.data(),
                                                    got.size(), mode, &word)
                                  : hostemu_csi_bed(bytes.data(), n, sizes.data(), n_blocks, base, (uint32_t)depth, got.data(), got.size(), mode, &word);
      if (r != (long)want_len || memcmp(got.data(), want.data(), want_len)) {
        printf("csi: %s, mode %d: %ld bytes, want %llu, or other bytes\n", argv[a], mode, r, (unsigned long long)want_len);
        return 1;
      }
    }
    printf("csi: %s: depth %llu, %llu bytes of index, four modes equal\n", argv[a], (unsigned long long)depth, (unsigned long long)want_len);
  }
  return 0;
}
