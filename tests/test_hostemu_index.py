"""Chunked reference-minimizer collection used by the device index builder
(cm_ref_chunk_minimizers in cm_stages.h) must emit exactly what the sequential state
machine emits (oracle: ora_minimizers == minimizer_generator.cc:7-139), and the builder's
table-sizing rule (sy_buckets_for) must be khash's."""
import ctypes as C

import numpy as np
import pytest

import datasets
import hostemu_lib as he
import index_refs
import oracle_lib as ol
from chromap_amd import _capi


@pytest.mark.parametrize("case,chunk,warm", [("s4_atac_q0", 2048, 96), ("s4_atac_q0", 257, 40), ("s1_atac", 2048, 96),
                                               ("toy_chip", 1000, 31)])
def test_chunked_reference_minimizers(case, chunk, warm):
    fa, _, _ = datasets.case_inputs(case)
    L = he.lib()
    L.hostemu_ref_minimizers.restype = C.c_long
    L.hostemu_ref_minimizers.argtypes = [C.POINTER(_capi.RefView), C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_long]
    ref = _capi.RefView()
    assert L.cmgpu_load_reference_fasta(fa.encode(), C.byref(ref)) == 0
    total = sum(ref.lengths[i] for i in range(ref.n_sequences))
    h = np.zeros(total, np.uint64)
    t = np.zeros(total, np.uint64)
    n = L.hostemu_ref_minimizers(C.byref(ref), 17, 7, chunk, warm, h.ctypes.data, t.ctypes.data, total)
    assert n > 0
    O = ol.lib()
    oh_all, ot_all = [], []
    for r in range(ref.n_sequences):
        ln = ref.lengths[r]
        oh = np.zeros(ln + 1, np.uint64)
        ot = np.zeros(ln + 1, np.uint64)
        seq = C.string_at(ref.sequences[r], ln)
        c = O.ora_minimizers(seq, ln, r, 17, 7, oh.ctypes.data, ot.ctypes.data)
        oh_all.append(oh[:c])
        ot_all.append(ot[:c])
    oh = np.concatenate(oh_all)
    ot = np.concatenate(ot_all)
    assert n == len(oh)
    # same multiset of (hash, hit); the builder sorts by (hash, hit) afterwards
    a = np.lexsort((t[:n], h[:n]))
    b = np.lexsort((ot, oh))
    assert np.array_equal(h[:n][a], oh[b]) and np.array_equal(t[:n][a], ot[b])
    L.cmgpu_free_host_ref(C.byref(ref))


# (28, 32) sits at the edge of the odd-k warm-up rule 2w + k = 92 <= 96; even k takes the path that counts window advances
KW_GRID = [(17, 7), (16, 7), (15, 5), (21, 11), (22, 10), (27, 7), (28, 32), (28, 7), (2, 1), (1, 1)]


def _chunked(seqs, k, w, chunk, warm):
    """the chunked pass over [(name, bytes)]: per sequence, (hash, hit) sorted by (hash, hit)"""
    L = he.lib()
    L.hostemu_ref_minimizers.restype = C.c_long
    L.hostemu_ref_minimizers.argtypes = [C.POINTER(_capi.RefView), C.c_int, C.c_int, C.c_uint32, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_long]
    rv, keep = index_refs.ref_view(seqs)
    total = sum(len(s) for _, s in seqs) + len(seqs)
    h = np.zeros(total, np.uint64)
    t = np.zeros(total, np.uint64)
    n = L.hostemu_ref_minimizers(C.byref(rv), k, w, chunk, warm, h.ctypes.data, t.ctypes.data, total)
    assert n >= 0
    h, t = h[:n], t[:n]
    rid = (t >> np.uint64(33)).astype(np.int64)
    out = []
    for r in range(len(seqs)):
        hh, tt = h[rid == r], t[rid == r]
        o = np.lexsort((tt, hh))
        out.append((hh[o], tt[o]))
    return out


def _sequential(seqs, k, w):
    O = ol.lib()
    out = []
    for r, (_, s) in enumerate(seqs):
        oh = np.zeros(len(s) + 1, np.uint64)
        ot = np.zeros(len(s) + 1, np.uint64)
        c = O.ora_minimizers(s, len(s), r, k, w, oh.ctypes.data, ot.ctypes.data)
        o = np.lexsort((ot[:c], oh[:c]))
        out.append((oh[:c][o], ot[:c][o]))
    return out


def _same_lists(got, want):
    """per sequence the same LIST of (hash, hit): a duplicated emission differs as a missing one does"""
    bad = []
    for r, ((gh, gt), (wh, wt)) in enumerate(zip(got, want)):
        if not (len(gh) == len(wh) and np.array_equal(gh, wh) and np.array_equal(gt, wt)):
            g = set(zip(gh.tolist(), gt.tolist()))
            x = set(zip(wh.tolist(), wt.tolist()))
            bad.append((r, len(gh), len(wh), sorted((t >> 1) & 0xffffffff for _, t in x - g)[:8],
                        sorted((t >> 1) & 0xffffffff for _, t in g - x)[:8]))
    return bad


@pytest.mark.parametrize("chunk,warm", [(2048, 96), (257, 96)])
@pytest.mark.parametrize("k,w", KW_GRID)
def test_chunked_minimizers_edge_reference(k, w, chunk, warm):
    seqs = index_refs.edge_reference(k, w)
    want = _sequential(seqs, k, w)
    assert sum(len(h) for h, _ in want) > 0
    bad = _same_lists(_chunked(seqs, k, w, chunk, warm), want)
    assert not bad, "sequence, emitted, expected, positions missing, positions in excess: %r" % bad


@pytest.mark.parametrize("k,w", KW_GRID)
def test_chunked_minimizers_placement_sweep(k, w):
    """one palindromic tandem run around the first chunk seam, 360 placements"""
    differ = []
    for unit, start, length, s in index_refs.placement_sweep():
        seqs = [(b"sweep", s)]
        if _same_lists(_chunked(seqs, k, w, 2048, 96), _sequential(seqs, k, w)):
            differ.append((unit, start, length))
    assert not differ, "%d of 360 placements differ, first %r" % (len(differ), differ[:5])


def test_chunked_minimizers_small_k_fuzz():
    """short k-mers make palindromes frequent, small chunks and warm-ups make every seam case frequent: random sequences with
    tandem runs and runs of N written over them, among them runs of N with a palindrome forming across them (the k-mer register
    keeps the bases in front of an ambiguous one)"""
    rng = np.random.RandomState(1)
    units = [b"AT", b"CG", b"ACGT", b"N", b"TA", b"GATC"]
    differ = []
    for it in range(400):
        k = int(rng.choice([2, 4, 6, 8, 10, 16]))
        w = int(rng.choice([1, 2, 3, 5, 7, 12]))
        n = int(rng.randint(1, 900))
        p = rng.dirichlet([1, 1, 1, 1, rng.choice([0.05, 0.5, 3])])
        a = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, n, p=p)].copy()
        for _ in range(rng.randint(0, 6)):
            st, ln = rng.randint(0, n), rng.randint(1, 200)
            u = units[rng.randint(len(units))]
            seg = np.frombuffer((u * (ln // len(u) + 1))[:ln], np.uint8)[:n - st]
            a[st:st + len(seg)] = seg
        chunk, warm = int(rng.choice([16, 64, 257])), int(rng.choice([1, 8, 16, 40, 96]))
        seqs = [(b"fuzz", bytes(a))]
        if _same_lists(_chunked(seqs, k, w, chunk, warm), _sequential(seqs, k, w)):
            differ.append((it, k, w, chunk, warm))
    assert not differ, differ[:5]


@pytest.mark.parametrize("k,w", KW_GRID)
def test_oracle_accepts_edge_reference(k, w, tmp_path):
    """every crafted input stays inside what the oracle accepts: it loads the FASTA as written and builds an index"""
    seqs = index_refs.edge_reference(k, w)
    fa = index_refs.write_fasta(str(tmp_path / "edge.fa"), seqs)
    O = ol.lib()
    ref = ol.OraRef()
    assert O.ora_ref_load(fa.encode(), C.byref(ref)) == 0
    assert ref.n_seq == len(seqs)
    for i, (name, s) in enumerate(seqs):
        assert ref.name[i] == name and ref.len[i] == len(s) and C.string_at(ref.seq[i], len(s)).upper() == s.upper()
    idx = ol.OraIndex()
    assert O.ora_index_build(C.byref(ref), k, w, C.byref(idx)) == 0
    assert idx.n_keys > 0 and idx.n_buckets >= 4
    O.ora_index_free(C.byref(idx))
    O.ora_ref_free(C.byref(ref))


# ---- the table-sizing rule ------------------------------------------------------------------
def _upper_bound(nb):
    return int(nb * 0.77 + 0.5) & 0xffffffff   # (khint_t)(n_buckets * __ac_HASH_UPPER + 0.5)


def _grow(nb):
    """kh_resize(h, n_buckets + 1): the next power of two, at least 4; 0 when that does not fit khash's 32 bits"""
    n = 4
    while n < nb + 1:
        n <<= 1
    return n if n < 1 << 32 else 0


def _khash_buckets_stepwise(n_max):
    """n_buckets after 0 .. n_max insertions of distinct keys into an empty khash, one kh_put at a time"""
    nb = occ = 0
    out = [0]
    for _ in range(n_max):
        if occ >= _upper_bound(nb):
            nb = _grow(nb)
        occ += 1
        out.append(nb)
    return out


def _khash_buckets(n):
    """the same rule, jumping from growth to growth"""
    nb = occ = 0
    while occ < n:
        nb = _grow(nb)
        if nb == 0:
            return 0
        occ = min(n, _upper_bound(nb))
    return nb


def test_buckets_for_is_khash_sizing():
    L = he.lib()
    L.hostemu_buckets_for.restype = C.c_uint32
    L.hostemu_buckets_for.argtypes = [C.c_uint64]
    step = _khash_buckets_stepwise(200000)
    assert step[1] == 4 and step[3] == 4 and step[4] == 8 and step[6] == 8 and step[7] == 16 and step[13] == 32
    # an index always has a key (the builder refuses a reference without one); for 0 keys the function answers khash's minimum
    assert L.hostemu_buckets_for(0) == 4
    got = [L.hostemu_buckets_for(n) for n in range(1, 200001)]
    assert got == step[1:]
    assert [_khash_buckets(n) for n in range(1, 200001)] == step[1:]
    nb, last = 4, None
    while nb < 1 << 32:
        ub = _upper_bound(nb)
        for n in range(max(1, ub - 3), ub + 5):    # ub keys still fit nb buckets, the next one doubles them
            assert L.hostemu_buckets_for(n) == _khash_buckets(n), (nb, n)
        last = ub
        nb <<= 1
    assert L.hostemu_buckets_for(last) == 1 << 31 and L.hostemu_buckets_for(last + 1) == 0
