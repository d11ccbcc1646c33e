"""The stage functions of the front end's planes route (chromap_amd/csrc/cm_stages.h; what k_prep_mm runs for batches whose longest read
has at most 64 bases: every read converted to bit planes once, cm_read_planes64, for the trim, the minimizer pass and the planes the
verification aligns on), compiled for the host (tests/hostemu/hostemu_pack_once.cpp):
  planes      cm_read_planes64 + cm_finish_read_planes against the byte definition, every length, alignment and trimmed length;
  trim        cm_trim_planes64 inside cm_s0_prep_ptr against the oracle's restatement of Chromap::TrimAdapterForPairedEndRead;
  minimizers  the planes source against the byte source and the oracle's GenerateMinimizers, k = 17, w = 7;
and the same sweeps in a stand-alone program under AddressSanitizer / UndefinedBehaviorSanitizer (shifts by 64, 64-bit masks)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import datasets
import oracle_lib as ol
from hostemu_pack_once_lib import lib, sanitizer_program

ALPHABET = b"ACGTacgtNn@[`{\x00\xff"
COMP = bytes.maketrans(b"ACGTNacgtn", b"TGCANtgcan")
AD1 = b"CTGTCTCTTATACACATCTCCGAGCCCACGAGACTAAGGCGAATCTCGTATGCCGTCTTCTGCTTG" * 2
AD2 = b"CTGTCTCTTATACACATCTGACGCTGCCGACGAGTGTAGATCTCGGTGGTCGCCGTATCATTAAAA" * 2
MIN_OVERLAP, SEED = 30, 15  # the atac preset: min_read_length 30, seeds of half that


# ---------------------------------------------------------------- planes
def run_planes(pool):
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    bad = (C.c_uint32 * 4)()
    rc = lib().hostemu_po_planes_check(pool.ctypes.data, len(pool), bad)
    assert rc >= 0, "planes differ (rc %d) at length %d, alignment %d, L / base %d, W %d" % (rc, bad[0], bad[1], bad[2], bad[3])
    return rc


def test_planes_of_every_length_alignment_and_trimmed_length():
    rng = np.random.default_rng(20261019)
    letters = np.frombuffer(ALPHABET, np.uint8)
    p = np.array([8] * 8 + [1] * (len(letters) - 8), float)  # mostly letters, every other byte often enough to land on every lane of a word
    assert run_planes(rng.choice(letters, 1 << 14, p=p / p.sum())) >= 16 * sum(L + 1 for L in range(1, 65))


def test_planes_of_every_byte_value():
    rng = np.random.default_rng(7)
    pool = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), 1 << 14)
    pool[::3] = np.arange(len(pool[::3])) % 256
    run_planes(pool)


# ---------------------------------------------------------------- trim
def mutate(rng, t, lo, hi):
    """one substitution in t[lo:hi)"""
    p = int(rng.integers(lo, hi))
    t[p] = ord("ACGT"[(b"ACGT".index(t[p]) + 1 + int(rng.integers(0, 3))) % 4])


def adversarial_pairs(seed):
    """mate lengths 30..64, equal and unequal; every overlap length from 2 below the minimum to 64; 0..3 mismatches inside seed 0,
    inside seed 1, outside both; N, lower case, AC / GT repeats; mates of 65 bases"""
    rng = np.random.default_rng(seed)
    r1s, r2s = [], []
    def add(a, b):
        r1s.append(bytes(a)); r2s.append(bytes(b))
    for fl in range(MIN_OVERLAP - 2, 65):
        for rep in range(24):
            l1 = int(rng.integers(30, 65))
            l2 = l1 if rep % 2 else int(rng.integers(30, 65))
            if rep % 8 == 0:
                l2 = 64
            if rep % 8 == 2:
                l1 = l2 = max(fl, 30)  # the overlap starts at the first base of the reverse complement
            frag = bytes(rng.choice(list(b"ACGT"), fl).astype(np.uint8))
            a = bytearray((frag + AD1)[:l1])
            b = bytearray((frag.translate(COMP)[::-1] + AD2)[:l2])
            nmut, where = rep % 4, (rep // 4) % 3
            span = min(fl, l1, l2)
            for _ in range(nmut):
                if where == 0:
                    mutate(rng, a, 0, min(SEED, span))
                elif where == 1:
                    mutate(rng, a, min(SEED, span - 1), min(2 * SEED, span))
                elif span > 2 * SEED:
                    mutate(rng, a if rng.random() < 0.5 else b, 2 * SEED, span)
            add(a, b)
            v = rep % 6
            t = bytearray(a) if rng.random() < 0.5 else bytearray(b)
            other_is_b = t == a
            if v == 0:
                t[int(rng.integers(0, len(t)))] = ord("N")
            elif v == 1:
                p = int(rng.integers(0, len(t))); t[p] |= 0x20
            elif v == 2:
                t = bytearray(bytes(t).lower())
            elif v == 3:
                add((b"AC" * 40)[:l1], (b"GT" * 40)[:l2]); continue
            elif v == 4:
                add(a, (frag.translate(COMP)[::-1] + AD2)[:65]); continue
            else:
                add((frag + AD1)[:65], b); continue
            add(t, b) if other_is_b else add(a, t)
    return r1s, r2s


def pack(ss):
    off = np.zeros(len(ss) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in ss])
    return np.concatenate([np.frombuffer(b"".join(ss), np.uint8), np.zeros(16, np.uint8)]), off


@pytest.mark.parametrize("seed,minlen", [(1, 30), (2, 31), (3, 40)])
def test_trim_on_planes_matches_oracle(seed, minlen):
    from chromap_amd import _capi
    r1s, r2s = adversarial_pairs(seed)
    b1, o1 = pack(r1s)
    b2, o2 = pack(r2s)
    fa, _, _ = datasets.case_inputs("toy_atac")
    o = ol.Oracle(datasets.case_index("toy_atac"), fa, ol.params("atac", min_read_length=minlen))
    _, _, _, tr = o.map_pairs(b1, o1, b2, o2, trace=True)
    p = _capi.default_params("atac", min_read_length=minlen)
    n = len(r1s)
    bt = _capi.Batch(n, 0, b1.ctypes.data, o1.ctypes.data, b2.ctypes.data, o2.ctypes.data)
    rlen = np.zeros(2 * n, np.uint32)
    n_planes = C.c_uint32(0)
    assert lib().hostemu_po_trim(C.addressof(p), C.addressof(bt), rlen.ctypes.data, C.byref(n_planes)) == 0
    trimmed = 0
    for i in range(n):
        if len(r1s[i]) < minlen or len(r2s[i]) < minlen:
            assert (rlen[2 * i], rlen[2 * i + 1]) == (0, 0)
            continue
        assert (rlen[2 * i], rlen[2 * i + 1]) == (tr[i].len1, tr[i].len2), (i, r1s[i], r2s[i])
        trimmed += rlen[2 * i] != len(r1s[i]) or rlen[2 * i + 1] != len(r2s[i])
    # coverage of the sweep itself: most pairs are upper-case ACGT; two in five carry at most one mismatch and, at the largest minimum
    # run here (40), two thirds of the fragment lengths still overlap far enough to be trimmed
    assert n_planes.value > n // 2 and trimmed > n // 8
    o.close()


# ---------------------------------------------------------------- minimizers
K, W = 17, 7


def minimizers(read, route, align=0):
    s = np.frombuffer(bytes(read), np.uint8)
    oh, op = np.zeros(80, np.uint64), np.zeros(80, np.uint32)
    n = lib().hostemu_po_minimizers(s.ctypes.data, len(s), K, route, align, oh.ctypes.data, op.ctypes.data, 80)
    assert n >= 0
    return [(int(h), int(p)) for h, p in zip(oh[:n], op[:n])]


def oracle_minimizers(read):
    s = np.concatenate([np.frombuffer(bytes(read), np.uint8), np.zeros(8, np.uint8)])
    oh, ot = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    n = ol.lib().ora_minimizers(s.ctypes.data_as(C.c_char_p), len(read), 0, K, W, oh.ctypes.data, ot.ctypes.data)
    return [(int(h), int(t) & 0xFFFFFFFF) for h, t in zip(oh[:n], ot[:n])]  # hit: sequence id << 32 | position << 1 | strand


def minimizer_reads():
    rng = np.random.default_rng(19)
    out = []
    for L in range(K, 65):
        for _ in range(6):
            out.append(bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8)))
        for c in b"ACGT":
            out.append(bytes([c]) * L)                                  # equal hashes in every window
        for u in (b"AC", b"GT", b"AT", b"CG", b"ACG", b"AACCT"):
            out.append((u * 64)[:L])                                    # ties at a distance: the first-window rule
        r = bytearray(rng.choice(list(b"ACGT"), L).astype(np.uint8))
        for pos in (0, K - 1, L // 2, L - 1):                           # N in the first k-mer, its last base, the middle, the last base
            t = bytearray(r); t[pos] = ord("N"); out.append(bytes(t))
        t = bytearray(r); t[L // 3] |= 0x20; out.append(bytes(t))       # lower case is a letter
    for L in range(1, K):
        out.append(bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8)))
    return out


def test_minimizers_from_planes_match_bytes_and_oracle():
    few = 0
    for i, read in enumerate(minimizer_reads()):
        got = minimizers(read, 0, align=i % 16)
        assert got == minimizers(read, 1), read
        assert got == minimizers(read, 2), read
        assert got == oracle_minimizers(read), read
        few += K <= len(read) < K + 6
    assert few > 50  # reads with fewer than seven k-mers: the flush rule


# ---------------------------------------------------------------- sanitizers
def test_sweeps_under_address_and_undefined_sanitizers():
    r = subprocess.run([sanitizer_program()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "all sweeps equal" in r.stdout, r.stdout[-4000:]
