"""The front end's planes route on the device (k_prep_mm's planes instance: batches whose longest read has at most 64 bases are converted
to bit planes once, for the trim, the minimizer pass and the planes the verification aligns on; no k_pack_reads) against the route it
replaces, cmgpu_set_option "pack_once" 1 and 0, one lane: records, trimmed lengths, every read's minimizer list (through mm_cnt /
mm_off: the blocks reserve their ranges in any order) and the plane words of every read that is left after trimming must be equal.
Shapes: around the 128 pairs of a block, two front-end chunks, mixed lengths 30..64 with the adversarial trim pairs of
tests/test_pack_once_cpu.py and reads with N, and a batch with one read of 65 bases, which both settings run on the old kernels."""
import ctypes as C

import numpy as np
import pytest

import fuzz_data
import oracle_lib as ol
import test_pack_once_cpu as cpu

pytestmark = pytest.mark.gpu

ACGT, COMP = fuzz_data.ACGT, fuzz_data.COMP
AD1 = np.frombuffer(cpu.AD1, np.uint8)
AD2 = np.frombuffer(cpu.AD2, np.uint8)
_G = {}


def _pack(rs):
    off = np.zeros(len(rs) + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rs])
    return np.frombuffer(b"".join(rs), np.uint8).copy(), off


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    """a genome of 300 kb, its index, one device context for the module"""
    from chromap_amd import ChromapGPU
    d = tmp_path_factory.mktemp("pack_once")
    rng = np.random.default_rng(20261019)
    chroms = [ACGT[rng.integers(0, 4, 100_000)].copy() for _ in range(3)]
    fa = str(d / "g.fa")
    with open(fa, "wb") as f:
        for i, c in enumerate(chroms):
            f.write(b">c%d\n" % i + c.tobytes() + b"\n")
    kw = {"mapq_threshold": 0}
    o = ol.Oracle(None, fa, ol.params("atac", **kw))
    idx = str(d / "g.idx")
    assert o.L.ora_index_save(idx.encode(), C.byref(o.idx)) == 0
    o.close()
    g = ChromapGPU(idx, fa, preset="atac", **kw)
    g.set_option("lanes", 1)
    _G["chroms"] = chroms
    yield g
    g.close()


def fragment_pairs(rng, n, lengths, n_rate=0.0):
    """pairs off fragments of 25..300 bases (the short ones run into the adapters: trimmed), 1 % substitutions; lengths: per read"""
    chroms = _G["chroms"]
    r1, r2 = [], []
    for i in range(n):
        fl = int(rng.integers(25, 300)) if i % 3 else int(rng.integers(25, 70))
        ci, st = int(rng.integers(0, 3)), int(rng.integers(0, 100_000 - fl))
        frag = chroms[ci][st:st + fl]
        la, lb = lengths(rng)
        a = np.concatenate([frag, AD1])[:la].copy()
        b = np.concatenate([COMP[frag[::-1]], AD2])[:lb].copy()
        for x in (a, b):
            m = rng.random(len(x)) < 0.01
            x[m] = ACGT[rng.integers(0, 4, int(m.sum()))]
            if rng.random() < n_rate:
                x[int(rng.integers(0, len(x)))] = ord("N")
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a.tobytes()); r2.append(b.tobytes())
    return r1, r2


def run(g, batch, on):
    """one mapping: what the two settings are compared by"""
    b1, o1, b2, o2 = batch
    n = len(o1) - 1
    g.set_option("pack_once", on)
    g.upload(b1, o1, b2, o2)
    k = g.map_resident()
    rec, k2 = g.download_records(max(1, k))
    assert k2 == k
    out = {"records": bytes(C.string_at(C.addressof(rec), 24 * k))}
    from chromap_amd import _capi
    out["rlen"] = _capi.debug_array(g.L, g.ctx, "rlen", n).copy()
    cnt, off = np.zeros(2 * n, np.uint32), np.zeros(2 * n, np.uint32)
    tot = C.c_uint64(0)
    cap = 2 * n * 70
    mh, mp = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
    assert g.L.cmgpu_debug_minimizers_all(g.ctx, cnt.ctypes.data, off.ctypes.data, mh.ctypes.data, mp.ctypes.data, cap, C.byref(tot)) == 0, g.L.cmgpu_last_error(g.ctx)
    total = int(cnt.sum())
    assert total == tot.value
    start = np.cumsum(cnt, dtype=np.int64) - cnt
    at = np.repeat(off.astype(np.int64), cnt) + (np.arange(total) - np.repeat(start, cnt))  # every read's list, in read order
    out["mm_cnt"], out["mm_hash"], out["mm_ps"] = cnt, mh[at], mp[at]
    longest = int(max(np.diff(o1.astype(np.int64)).max(), np.diff(o2.astype(np.int64)).max()))
    W = (longest + 31) // 32
    stride = (6 * W + 3) & ~3
    pl = np.zeros(2 * n * stride, np.uint32)
    nw = C.c_uint64(0)
    assert g.L.cmgpu_debug_array(g.ctx, b"read_pl", pl.ctypes.data, len(pl), C.byref(nw)) == 0, g.L.cmgpu_last_error(g.ctx)
    assert nw.value == len(pl)
    pl = pl.reshape(2 * n, stride)
    pl[out["rlen"] == 0] = 0  # (nothing is written for a read that was filtered out)
    out["read_pl"], out["W"] = pl, W
    return out


def check_forward_planes(batch, res, sample):
    """the forward planes of some reads against their bytes: base i = bit i of p0 (code & 1), p1 (code >> 1), pn (no base, or past the end)"""
    b1, o1, b2, o2 = batch
    W = res["W"]
    for r in sample:
        b, o = (b2, o2) if r & 1 else (b1, o1)
        L = int(res["rlen"][r])
        if L == 0:
            continue
        seq = bytes(b[o[r >> 1]:o[r >> 1] + L]).upper()
        want = [0, 0, 0]
        for i in range(32 * W):
            c = b"ACGT".find(seq[i:i + 1]) if i < L else -1
            if c < 0:
                want[2] |= 1 << i
            else:
                want[0] |= (c & 1) << i
                want[1] |= (c >> 1) << i
        for q in range(3):
            got = sum(int(res["read_pl"][r, q * W + w]) << (32 * w) for w in range(W))
            assert got == want[q], (r, q)


def compare(g, batch, planes_route=True):
    assert g.get_option("pack_once") in (0, 1)
    a, b = run(g, batch, 1), run(g, batch, 0)
    for what in ("records", "rlen", "mm_cnt", "mm_hash", "mm_ps", "read_pl"):
        same = a[what] == b[what] if what == "records" else np.array_equal(a[what], b[what])
        assert same, what
    n2 = len(a["rlen"])
    check_forward_planes(batch, a, range(0, n2, max(1, n2 // 97)))
    return a


@pytest.mark.parametrize("n", [1, 127, 128, 129, 257])
def test_around_a_block_of_pairs(gpu, n):
    rng = np.random.default_rng(n)
    r1, r2 = fragment_pairs(rng, n, lambda rng: (50, 50))
    res = compare(gpu, _pack(r1) + _pack(r2))
    assert n < 100 or (res["rlen"] > 0).sum() > n


def test_two_front_end_chunks(gpu):
    rng = np.random.default_rng(131077)
    r1, r2 = fragment_pairs(rng, 4096, lambda rng: (50, 50))
    pick = rng.integers(0, 4096, 131_077)
    res = compare(gpu, _pack([r1[i] for i in pick]) + _pack([r2[i] for i in pick]))
    assert len(res["records"]) > 24 * 60_000 and ((res["rlen"] > 0) & (res["rlen"] < 50)).sum() > 20_000  # mapped, and trimmed


def test_mixed_lengths_adversarial_trims_and_n(gpu):
    rng = np.random.default_rng(64)
    r1, r2 = fragment_pairs(rng, 18_000, lambda rng: (int(rng.integers(30, 65)), int(rng.integers(30, 65))), n_rate=0.01)  # 2 % of the pairs with an N
    a1, a2 = cpu.adversarial_pairs(9)
    keep = [i for i in range(len(a1)) if len(a1[i]) <= 64 and len(a2[i]) <= 64]
    r1 += [a1[i] for i in keep]; r2 += [a2[i] for i in keep]
    r1, r2 = (r1 * 2)[:20_000], (r2 * 2)[:20_000]
    r1[-1] = r1[-1][:30] + b"ACGTACGTACGTACGTACGTACGTACGTACGTAC"  # the longest read has 64 bases
    assert max(map(len, r1 + r2)) == 64 and len(r1) == 20_000
    res = compare(gpu, _pack(r1) + _pack(r2))
    assert res["W"] == 2 and ((res["rlen"] > 0) & (res["rlen"] <= 32)).sum() > 100  # reads of one word in a batch of two


def test_a_read_of_65_bases_keeps_the_old_kernels(gpu):
    rng = np.random.default_rng(65)
    r1, r2 = fragment_pairs(rng, 3000, lambda rng: (int(rng.integers(30, 65)), int(rng.integers(30, 65))), n_rate=0.01)
    r1[1500] = (r1[1500] + cpu.AD1)[:65]
    res = compare(gpu, _pack(r1) + _pack(r2))
    assert res["W"] == 3 and (res["rlen"] > 0).sum() > 3000
