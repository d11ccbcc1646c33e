// Stand-alone run of the planes route's three sweeps (hostemu_pack_once.cpp) for a sanitizer build -- the shifts by 64 and the 64-bit
// masks are what it is for (L = 32 and 64, an overlap at s0 = 0, a mate of 64 bases):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-strict-aliasing
//       tests/hostemu/pack_once_san_main.cpp -o pack_once_san && ./pack_once_san
// tests/test_pack_once_cpu.py builds and runs it.  Everything is compared inside the program: planes against the byte definition, the
// trim on planes against the trim on bytes, the minimizers from planes against the state machine.  Exit status 0: all equal.
#include <stdio.h>

#include <string>

#include "hostemu_pack_once.cpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*, a number below n
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}
static std::string random_bases(uint32_t n) {
  std::string s(n, 'A');
  for (auto &c : s) c = "ACGT"[rnd(4)];
  return s;
}
static std::string revcomp(const std::string &s) {
  std::string r(s.rbegin(), s.rend());
  for (auto &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
  return r;
}

static int sweep_planes() {
  static const char alphabet[] = "ACGTacgtNn@[`{\x00\xff";
  std::vector<uint8_t> pool(1 << 14);
  for (auto &b : pool) b = (uint8_t)(rnd(3) ? "ACGTacgt"[rnd(8)] : alphabet[rnd(16)]);
  uint32_t bad[4] = {0, 0, 0, 0};
  const long rc = hostemu_po_planes_check(pool.data(), (uint32_t)pool.size(), bad);
  if (rc < 0) { fprintf(stderr, "planes: rc %ld at len %u align %u L %u W %u\n", rc, bad[0], bad[1], bad[2], bad[3]); return 1; }
  printf("planes: %ld cases\n", rc);
  return 0;
}

static int sweep_trim() {
  const std::string ad1 = "CTGTCTCTTATACACATCTCCGAGCCCACGAGACTAAGGCGAATCTCGTATGCCGTCTTCTGCTTG", ad2 = "CTGTCTCTTATACACATCTGACGCTGCCGACGAGTGTAGATCTCGGTGGTCGCCGTATCATTAAAA";
  std::string b1, b2;
  std::vector<uint32_t> o1(1, 0), o2(1, 0);
  const uint32_t n = 20000;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t l1 = 30 + rnd(35), l2 = rnd(2) ? l1 : 30 + rnd(35);
    if (i % 16 == 0) l2 = 64;            // the 64-bit edges: a mate of 64 bases,
    if (i % 32 == 0) l1 = 64;
    uint32_t fl = 26 + rnd(45);
    if (i % 8 == 1) fl = l1 > l2 ? l1 : l2;  // an overlap that starts at s0 = 0
    const std::string frag = random_bases(fl);
    std::string a = (frag + ad1 + ad1).substr(0, l1), b = (revcomp(frag) + ad2 + ad2).substr(0, l2);
    for (uint32_t m = rnd(4); m > 0; --m) {
      std::string &t = rnd(2) ? a : b;
      const uint32_t p = rnd((uint32_t)t.size());
      t[p] = t[p] == 'A' ? 'C' : 'A';
    }
    const uint32_t v = rnd(100);
    if (v < 5) { std::string &t = rnd(2) ? a : b; t[rnd((uint32_t)t.size())] = 'N'; }
    else if (v < 10) { std::string &t = rnd(2) ? a : b; const uint32_t p = rnd((uint32_t)t.size()); t[p] = (char)(t[p] | 0x20); }
    else if (v < 12) for (auto &c : a) c = (char)(c | 0x20);
    else if (v < 17) { a = std::string(); b = std::string(); for (uint32_t q = 0; q < l1; ++q) a += "AC"[q & 1]; for (uint32_t q = 0; q < l2; ++q) b += "GT"[q & 1]; }
    else if (v < 19) b = (revcomp(frag) + ad2 + ad2).substr(0, 65);  // a mate of 65 bases: no planes
    b1 += a; b2 += b;
    o1.push_back((uint32_t)b1.size()); o2.push_back((uint32_t)b2.size());
  }
  b1 += std::string(16, 'A'); b2 += std::string(16, 'A');
  for (int minlen : {30, 31, 40, 64}) {
    cmgpu_params p;
    memset(&p, 0, sizeof p);
    p.min_read_length = minlen; p.trim_adapters = 1;
    cmgpu_batch bt;
    memset(&bt, 0, sizeof bt);
    bt.n_pairs = n; bt.read1_bases = b1.data(); bt.read1_offsets = o1.data(); bt.read2_bases = b2.data(); bt.read2_offsets = o2.data();
    std::vector<uint32_t> ra(2 * n), rb(2 * n);
    uint32_t n_planes = 0, trimmed = 0;
    hostemu_po_trim(&p, &bt, ra.data(), &n_planes);
    CmDev d;
    memset(&d, 0, sizeof d);
    d.p.min_read_len = minlen; d.p.trim = 1;
    d.rb0 = (const uint8_t *)b1.data(); d.rb1 = (const uint8_t *)b2.data(); d.ro0 = o1.data(); d.ro1 = o2.data(); d.rlen = rb.data();
    for (uint32_t i = 0; i < n; ++i) cm_s0_prep(d, i);
    for (uint32_t i = 0; i < 2 * n; ++i) {
      if (ra[i] != rb[i]) { fprintf(stderr, "trim: min length %d, read %u: %u on planes, %u on bytes\n", minlen, i, ra[i], rb[i]); return 1; }
      trimmed += ra[i] != 0 && ra[i] != ((i & 1) ? o2[i / 2 + 1] - o2[i / 2] : o1[i / 2 + 1] - o1[i / 2]);
    }
    printf("trim: min length %d, %u pairs on planes, %u reads trimmed\n", minlen, n_planes, trimmed);
    if (n_planes < n / 2 || (minlen <= 40 && trimmed < n / 8)) { fprintf(stderr, "trim: the sweep does not reach the planes route\n"); return 1; }
  }
  return 0;
}

static int sweep_minimizers() {
  long cases = 0;
  for (uint32_t len = 1; len <= 64; ++len)
    for (uint32_t kind = 0; kind < 24; ++kind) {
      std::string s = random_bases(len);
      if (kind == 1) s = std::string(len, "ACGT"[rnd(4)]);
      if (kind == 2 || kind == 3) { const char x = "ACGT"[rnd(4)], y = "ACGT"[rnd(4)]; for (uint32_t q = 0; q < len; ++q) s[q] = (q & 1) ? x : y; }
      if (kind == 4) { const std::string u = random_bases(3 + rnd(6)); for (uint32_t q = 0; q < len; ++q) s[q] = u[q % u.size()]; }
      if (kind == 5) s[0] = 'N';
      if (kind == 6) s[len - 1] = 'N';
      if (kind == 7) s[rnd(len)] = 'n';
      if (kind == 8) for (auto &c : s) c = (char)(c | 0x20);
      for (int k : {17, 15, 21, 18}) {
        uint64_t ha[80], hb[80];
        uint32_t pa[80], pb[80];
        const int na = hostemu_po_minimizers((const uint8_t *)s.data(), len, k, 0, rnd(16), ha, pa, 80);
        const int nb = hostemu_po_minimizers((const uint8_t *)s.data(), len, k, 2, rnd(16), hb, pb, 80);
        bool ok = na == nb;
        for (int i = 0; ok && i < na; ++i) ok = ha[i] == hb[i] && pa[i] == pb[i];
        if (!ok) { fprintf(stderr, "minimizers: k %d, read %s: %d from planes, %d from the state machine\n", k, s.c_str(), na, nb); return 1; }
        ++cases;
      }
    }
  printf("minimizers: %ld cases\n", cases);
  return 0;
}

int main() {
  if (sweep_planes() || sweep_trim() || sweep_minimizers()) return 1;
  printf("pack_once: all sweeps equal\n");
  return 0;
}
