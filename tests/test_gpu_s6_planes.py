"""S6's start positions from bit planes on the device (cm_ref_start_end: for a read of at most 64 bases made of upper-case A/C/G/T only,
the mismatch count in front of the traceback is taken on the planes the front end packed -- cm_hamming_diag_planes -- instead of on
bytes) against the byte route, cmgpu_set_option "s6_planes" 1 and 0, one lane: record bytes, the stage trace and pe_nbest must be equal.
The genome carries a soft-masked stretch and a run of N in every chromosome, and some fragments lie within the first and the last ten
bases of a chromosome (the window clamp).  Shapes: around a wave of 64 pairs, substitutions only and with one-base indels (the byte
traceback behind a failed count), mixed lengths 30..64, reads with N or lower-case bases (flag 0 for exactly those), a batch with one
read of 65 bases (every flag 0), one single-end and one --preset hic batch."""
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
CHR_LEN = 100_000
_G = {}


def _pack(rs):
    off = np.zeros(len(rs) + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rs])
    return np.frombuffer(b"".join(rs), np.uint8).copy(), off


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    """a genome of 300 kb in three chromosomes, each with 4 kb of lower-case letters and 200 N; its index; one device context"""
    from chromap_amd import ChromapGPU
    d = tmp_path_factory.mktemp("s6_planes")
    rng = np.random.default_rng(20261021)
    chroms = [ACGT[rng.integers(0, 4, CHR_LEN)].copy() for _ in range(3)]
    fa = str(d / "g.fa")
    with open(fa, "wb") as f:
        for i, c in enumerate(chroms):
            t = c.copy()
            lo = 30_000 + 1000 * i
            t[lo:lo + 4000] |= 0x20
            t[60_000:60_200] = ord("N")
            chroms[i][60_000:60_200] = ord("N")  # (fragments are cut from the upper-case text: sequencers do not report case)
            f.write(b">c%d\n" % i + t.tobytes() + b"\n")
    kw = {"mapq_threshold": 0}
    o = ol.Oracle(None, fa, ol.params("atac", **kw))
    idx = str(d / "g.idx")
    assert o.L.ora_index_save(idx.encode(), C.byref(o.idx)) == 0
    o.close()
    g = ChromapGPU(idx, fa, preset="atac", **kw)
    g.set_option("lanes", 1)
    _G.update(chroms=chroms, fa=fa, idx=idx, masked=[(30_000 + 1000 * i, 34_000 + 1000 * i) for i in range(3)])
    yield g
    g.close()


def _edit(rng, x, sub, indel):
    """substitutions at rate `sub`, one-base insertions / deletions at rate `indel` per base; the length is kept (cut or padded by the caller)"""
    out = []
    for c in x:
        u = rng.random()
        if u < indel / 2:
            continue                                  # a deletion
        if u < indel:
            out.append(int(ACGT[rng.integers(0, 4)]))  # an insertion
        out.append(int(ACGT[rng.integers(0, 4)]) if rng.random() < sub else int(c))
    return np.array(out, np.uint8)


def fragment_pairs(rng, n, lengths, indel=0.0, longer=300):
    """pairs off fragments of 25..`longer` bases, 1 % substitutions; one fragment in six starts within the first ten or ends within the
    last ten bases of its chromosome, one in six lies in the soft-masked stretch; lengths: per read"""
    chroms = _G["chroms"]
    r1, r2 = [], []
    for i in range(n):
        fl = int(rng.integers(25, longer)) if i % 3 else int(rng.integers(25, 70))
        ci = int(rng.integers(0, 3))
        if i % 6 == 1:
            st = int(rng.integers(0, 10)) if i % 12 == 1 else CHR_LEN - fl - int(rng.integers(0, 10))
        elif i % 6 == 4:
            st = int(rng.integers(_G["masked"][ci][0] - 40, _G["masked"][ci][1] - fl))
        else:
            st = int(rng.integers(0, CHR_LEN - fl))
        frag = chroms[ci][st:st + fl]
        la, lb = lengths(rng)
        a = np.concatenate([_edit(rng, frag, 0.01, indel), AD1])[:la].copy()
        b = np.concatenate([_edit(rng, COMP[frag[::-1]], 0.01, indel), AD2])[:lb].copy()
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a.tobytes()); r2.append(b.tobytes())
    return r1, r2


def _flags(g, n):
    out = np.zeros(max(1, 2 * n), np.uint32)
    k = C.c_uint64(0)
    assert g.L.cmgpu_debug_array(g.ctx, b"read_plain", out.ctypes.data, len(out), C.byref(k)) == 0, g.L.cmgpu_last_error(g.ctx)
    assert k.value == 2 * n
    return out[:2 * n]


def run(g, batch, on):
    from chromap_amd import _capi
    b1, o1, b2, o2 = batch
    n = len(o1) - 1
    g.set_option("s6_planes", on)
    assert g.get_option("s6_planes") == on
    rec, k = g.map_pairs(b1, o1, b2, o2)
    out = {"k": k, "records": bytes(C.string_at(C.addressof(rec), 24 * k))}
    gt = (ol.OraTrace * n)()  # cmgpu_trace has ora_trace's layout
    assert g.L.cmgpu_debug_trace(g.ctx, C.cast(gt, C.c_void_p), n) == 0, g.L.cmgpu_last_error(g.ctx)
    out["trace"] = bytes(C.string_at(C.addressof(gt), C.sizeof(gt)))
    out["gt"] = gt
    out["pe_nbest"] = _capi.debug_array(g.L, g.ctx, "pe_nbest", n).copy()
    if on:
        out["flags"] = _flags(g, n).copy()
    return out


def expected_flags(batch):
    b1, o1, b2, o2 = batch
    n = len(o1) - 1
    plain = np.zeros(256, bool)
    plain[list(b"ACGT")] = True
    f = np.zeros(2 * n, np.uint32)
    for i in range(n):
        f[2 * i] = plain[b1[o1[i]:o1[i + 1]]].all()
        f[2 * i + 1] = plain[b2[o2[i]:o2[i + 1]]].all()
    return f


def compare(g, batch, plane_route=True):
    assert g.get_option("s6_planes") in (0, 1)
    a, b = run(g, batch, 1), run(g, batch, 0)
    for what in ("k", "records", "trace"):
        assert a[what] == b[what], what
    assert np.array_equal(a["pe_nbest"], b["pe_nbest"])
    want = expected_flags(batch) if plane_route else np.zeros(len(a["flags"]), np.uint32)
    assert np.array_equal(a["flags"], want)
    g.set_option("s6_planes", 1)
    return a


def plain_reads_with_errors(res, n):
    """pairs with a record whose reads both carry flag 1 and of which one has a best mapping with errors: the planes arm counted there"""
    ids = set(np.frombuffer(res["records"], np.uint32).reshape(-1, 6)[:, 0].tolist())
    gt, fl = res["gt"], res["flags"]
    return sum(1 for i in range(n) if i in ids and fl[2 * i] and fl[2 * i + 1] and (gt[i].min_err1 > 0 or gt[i].min_err2 > 0))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_substitutions_around_a_wave(gpu, n):
    rng = np.random.default_rng(n)
    r1, r2 = fragment_pairs(rng, n, lambda rng: (50, 50))
    res = compare(gpu, _pack(r1) + _pack(r2))
    if n >= 63:
        assert res["k"] > n // 2
        # 1 - 0.99 ** 100 = 63 % of the pairs carry a substitution; adapters and soft-masked fragments add to that
        assert plain_reads_with_errors(res, n) > n // 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_one_base_indels_reach_the_byte_traceback(gpu, n):
    rng = np.random.default_rng(1000 + n)
    r1, r2 = fragment_pairs(rng, n, lambda rng: (50, 50), indel=0.005)
    res = compare(gpu, _pack(r1) + _pack(r2))
    if n >= 63:
        assert res["k"] > n // 2 and plain_reads_with_errors(res, n) > n // 4


def test_mixed_lengths(gpu):
    rng = np.random.default_rng(3064)
    r1, r2 = fragment_pairs(rng, 257, lambda rng: (int(rng.integers(30, 65)), int(rng.integers(30, 65))), indel=0.002)
    r1[-1] = (r1[-1] + cpu.AD1)[:64]
    res = compare(gpu, _pack(r1) + _pack(r2))
    assert max(map(len, r1 + r2)) == 64 and res["k"] > 128 and plain_reads_with_errors(res, 257) > 64


def test_reads_with_n_or_lower_case_keep_the_byte_route(gpu):
    rng = np.random.default_rng(78)
    r1, r2 = fragment_pairs(rng, 257, lambda rng: (50, 50))
    special = 0
    for rs in (r1, r2):
        for i in range(len(rs)):
            t = bytearray(rs[i])
            if i % 7 == 3:
                t[int(rng.integers(0, len(t)))] = ord("N"); special += 1
            elif i % 11 == 5:
                p = int(rng.integers(0, len(t))); t[p] |= 0x20; special += 1
            elif i % 13 == 6:
                t = bytearray(bytes(t).lower()); special += 1
            rs[i] = bytes(t)
    batch = _pack(r1) + _pack(r2)
    res = compare(gpu, batch)
    assert int((res["flags"] == 0).sum()) >= special > 100  # (a fragment over the genome's N run adds to them)
    assert res["k"] > 128 and plain_reads_with_errors(res, 257) > 32


def test_a_read_of_65_bases_clears_every_flag(gpu):
    rng = np.random.default_rng(65)
    r1, r2 = fragment_pairs(rng, 257, lambda rng: (int(rng.integers(30, 65)), int(rng.integers(30, 65))))
    r1[100] = (r1[100] + cpu.AD1)[:65]
    res = compare(gpu, _pack(r1) + _pack(r2), plane_route=False)
    assert res["k"] > 128 and not res["flags"].any()


def test_single_end(gpu):
    rng = np.random.default_rng(5)
    r1, r2 = fragment_pairs(rng, 257, lambda rng: (50, 50), indel=0.002)
    b, off = _pack(r1 + r2)
    out = {}
    for on in (1, 0):
        gpu.set_option("s6_planes", on)
        rec, k = gpu.map_single(b, off)
        out[on] = (k, bytes(C.string_at(C.addressof(rec), 24 * k)))
    gpu.set_option("s6_planes", 1)
    assert out[1] == out[0] and out[1][0] > 257


def test_preset_hic(gpu):
    from chromap_amd import ChromapGPU
    rng = np.random.default_rng(6)
    r1, r2 = fragment_pairs(rng, 257, lambda rng: (50, 50), indel=0.002)
    batch = _pack(r1) + _pack(r2)
    g = ChromapGPU(_G["idx"], _G["fa"], preset="hic", mapq_threshold=0)
    try:
        g.set_option("lanes", 1)
        out = {}
        for on in (1, 0):
            g.set_option("s6_planes", on)
            rec, k = g.map_pairs(*batch)
            out[on] = (k, bytes(C.string_at(C.addressof(rec), 24 * k)))
        assert out[1] == out[0] and out[1][0] > 64
    finally:
        g.close()
