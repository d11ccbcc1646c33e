"""The short-list form of S3b (cm_s3b_short, chromap_amd/csrc/cm_stages.h: hits of both strands in one list with the strand in bit 63,
a 16-key sorting network, one sweep, candidates straight to their slots) against the form that defines the stage (cm_s3b_core through
cm_s3b_candidates_lds: two lists, two insertion sorts, two sweeps), compiled for the host (tests/hostemu/hostemu_valu.cpp) and fed
synthetic lookup results directly: per minimizer a kind, a value and a position/strand word, plus the occurrence table.  Every array
the stage leaves -- hbuf and hcnt over the read's whole segment, n_pos_hit, ncp, ncn -- must be equal, element for element."""
import ctypes as C

import numpy as np

from hostemu_valu_lib import lib

MISS, SINGLE, MULTI = 0, 1, 2
K, W = 17, 7
MAX_ID = (1 << 31) - 2  # the largest sequence id the strand-in-bit-63 form is used with
U32 = 1 << 32


class Batch:
    """lookup results of a batch of reads, built hit by hit from the candidate each hit is to become"""
    def __init__(self, rng):
        self.rng = rng
        self.mm_off, self.kind, self.val, self.ps, self.occ = [0], [], [], [], []

    def ref_hit(self, rid, start, same, rp, sb):
        # inverse of cm_cand_from_hit: the occurrence whose candidate is (rid, start) on the strand `same` selects
        pos = (start + rp if same else start - rp + K - 1) % U32
        return (rid << 33) | (pos << 1) | (sb if same else 1 - sb)

    def minimizer(self, hits, single=False):
        """hits: [(rid, start, same)] of one minimizer, or None for a miss"""
        rp, sb = int(self.rng.integers(0, 34)), int(self.rng.integers(0, 2))
        self.ps.append((rp << 1) | sb)
        if hits is None:
            self.kind.append(MISS); self.val.append(int(self.rng.integers(0, 1 << 40)))
        elif single:
            assert len(hits) == 1
            self.kind.append(SINGLE); self.val.append(self.ref_hit(*hits[0], rp, sb))
        else:
            self.kind.append(MULTI); self.val.append((len(self.occ) << 32) | len(hits))
            self.occ.extend(self.ref_hit(*h, rp, sb) for h in hits)

    def end_read(self):
        self.mm_off.append(len(self.kind))

    def read(self, hits, n_mm=None, runs=None):
        """spreads `hits` over minimizers: `runs` gives the run lengths, else random ones; pads with misses up to n_mm minimizers"""
        rng = self.rng
        hits = list(hits)
        start = len(self.kind)
        if runs is None:
            runs = []
            left = len(hits)
            while left:
                c = int(min(left, rng.choice([1, 1, 1, 2, 3, 5])))
                runs.append(c); left -= c
        at = 0
        for c in runs:
            self.minimizer(hits[at:at + c], single=(c == 1 and rng.integers(0, 2) == 0))
            at += c
        assert at == len(hits)
        while len(self.kind) - start < (n_mm or 1):
            self.minimizer(None)
        self.end_read()

    def check(self, e, f0, f1, min_seeds):
        n = len(self.mm_off) - 1
        assert n % 2 == 0
        a = [np.asarray(self.mm_off, np.uint32), np.asarray(self.kind, np.uint8), np.asarray(self.val, np.uint64),
             np.asarray(self.ps, np.uint32), np.asarray(self.occ + [0], np.uint64)]
        tot, r2, nc = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        bad = C.c_long(-1)
        rc = lib().hostemu_s3b_short_check(n, *[x.ctypes.data for x in a], len(self.occ), e, K, W, f0, f1, min_seeds,
                                           tot.ctypes.data, r2.ctypes.data, nc.ctypes.data, C.byref(bad))
        assert rc >= 0, "read %d differs (rc %d): minimizers %s" % (bad.value, rc, self.describe(bad.value))
        return rc, tot, r2, nc

    def describe(self, r):
        lo, hi = self.mm_off[r], self.mm_off[r + 1]
        return [(self.kind[i], hex(self.val[i]), self.ps[i]) for i in range(lo, hi)]


def loci_hits(rng, n, e, ids, same=None, wrap=False):
    """n hits around a few loci, offsets of 0 .. e + 1, many exact repeats"""
    nl = int(rng.integers(1, 4))
    base = (U32 - 1 - rng.integers(0, 3 * e + 4, nl)) if wrap else rng.integers(0, 1 << 20, nl)
    out = []
    for _ in range(n):
        q = int(rng.integers(0, nl))
        s = (int(base[q]) + int(rng.integers(0, e + 2)) * int(rng.integers(0, 2))) % U32
        out.append((int(ids[q % len(ids)]), s, bool(rng.integers(0, 2)) if same is None else same))
    return out


def build(rng, n_reads, e, f0, f1):
    b = Batch(rng)
    modes = 12
    for r in range(n_reads):
        mode = r % modes
        n = int(rng.integers(0, 17))
        ids = [0, 1, 7, MAX_ID]
        rng.shuffle(ids)
        if mode == 0:      # a few loci on both strands
            b.read(loci_hits(rng, n, e, ids), n_mm=int(rng.integers(1, 10)))
        elif mode == 1:    # every hit on the + strand
            b.read(loci_hits(rng, n, e, ids, same=True), n_mm=int(rng.integers(1, 10)))
        elif mode == 2:    # every hit on the - strand
            b.read(loci_hits(rng, n, e, ids, same=False), n_mm=int(rng.integers(1, 10)))
        elif mode == 3:    # repeated identical hits: the best_equal bookkeeping (runs of equal hits that tie and that overtake)
            a, c = int(rng.integers(1, 6)), int(rng.integers(1, 6))
            s = int(rng.integers(0, 1 << 20))
            st = bool(rng.integers(0, 2))
            hits = [(5, s, st)] * a + [(5, s + int(rng.integers(1, e + 1)), st)] * c + [(5, s + 1, not st)] * int(rng.integers(0, 4))
            b.read(hits[:16], n_mm=int(rng.integers(1, 4)))
        elif mode == 4:    # one diagonal per strand with gaps of 0, 1, e and e + 1, few minimizers: the third break (mcount >= minimizers)
            hits = []
            for st in (True, False):
                s = np.cumsum(rng.choice([0, 1, e, e + 1], int(rng.integers(0, 9)))) + int(rng.integers(0, 1000))
                hits += [(3, int(x), st) for x in s]
            rng.shuffle(hits)
            b.read(hits, runs=[len(hits)] if hits and rng.integers(0, 2) and len(hits) < f0 else None, n_mm=int(rng.integers(1, 4)))
        elif mode == 5:    # several sequence ids, the largest among them, at the same positions
            s = int(rng.integers(0, 1 << 20))
            hits = [(int(rng.choice(ids)), s + int(rng.integers(0, 3)), bool(rng.integers(0, 2))) for _ in range(n)]
            b.read(hits, n_mm=int(rng.integers(1, 10)))
        elif mode == 6:    # positions at the u32 wrap of pos + e
            b.read(loci_hits(rng, n, e, ids, wrap=True), n_mm=int(rng.integers(1, 10)))
        elif mode == 7:    # a diagonal that wraps below zero: reference position smaller than the read's
            hits = [(int(rng.choice(ids)), (int(rng.integers(0, 4)) - int(rng.integers(0, 40))) % U32, True) for _ in range(n)]
            hits += [(2, int(rng.integers(0, 6)), bool(rng.integers(0, 2))) for _ in range(16 - n if n > 10 else 0)]
            b.read(hits[:16], n_mm=int(rng.integers(1, 10)))
        elif mode == 8:    # round 2: every run at or beyond the first limit and below the second (no hit in round 1)
            hits, runs = [], []
            while f1 > f0 and len(hits) + f0 <= 16 and rng.integers(0, 4):
                c = int(rng.integers(f0, min(f1, 16 - len(hits) + 1)))
                runs.append(c)
                hits += loci_hits(rng, c, e, ids)
            b.read(hits, runs=runs, n_mm=int(rng.integers(1, 6)))
        elif mode == 9:    # runs one below and at each frequency limit, next to short ones
            hits, runs = [], []
            for c in rng.permutation([f0 - 1, f0, f1 - 1, f1, 1, 2]):
                c = int(c)
                if 1 <= c <= 17 and rng.integers(0, 2):
                    runs.append(c)
                    hits += loci_hits(rng, c, e, ids)
            b.read(hits, runs=runs, n_mm=int(rng.integers(1, 8)))
        elif mode == 10:   # the totals at the ends of the range, exactly: 0, 1, 15, 16 (and 17: not this kernel's)
            t = int(rng.choice([0, 1, 15, 16, 17]))
            hits = loci_hits(rng, t, e, ids)
            b.read(hits, runs=[1] * t if rng.integers(0, 2) else None, n_mm=int(rng.integers(1, 20)))
        else:              # sparse: every hit a cluster of its own
            b.read([(int(rng.choice(ids)), int(rng.integers(0, U32)), bool(rng.integers(0, 2))) for _ in range(n)], n_mm=int(rng.integers(1, 10)))
    return b


def test_short_list_form_equals_the_defining_form():
    rng = np.random.default_rng(20261019)
    compared = 0
    seen_tot, seen_r2, seen_cand = set(), 0, 0
    # (e, f0, f1, min_seeds): the product's limits, and small ones so that lists of at most 16 hits meet them
    for e, f0, f1, ms in ((4, 500, 1000, 2), (4, 4, 9, 2), (8, 6, 12, 2), (3, 3, 3, 1), (15, 5, 16, 3), (1, 2, 17, 2)):
        b = build(rng, 4200, e, f0, f1)
        rc, tot, r2, nc = b.check(e, f0, f1, ms)
        compared += rc
        short = tot <= 16
        seen_tot |= set(int(x) for x in tot[short])
        seen_r2 += int((r2[short] & (tot[short] > 0)).sum())
        seen_cand += int(nc[short].sum())
    assert compared >= 20000, compared
    assert {0, 1, 15, 16} <= seen_tot, sorted(seen_tot)
    assert seen_r2 > 100, seen_r2      # round-2 reads with hits
    assert seen_cand > 20000, seen_cand  # and the lists are not empty
