"""The table the pipeline probes, looked at directly: the device index builder (cm_synth.hip: k_sy_ref_minimizers, the two radix
sorts, k_sy_flag_multi, the scans, k_sy_insert, sy_buckets_for, cmgpu_save_index_file), the re-pack of a loaded file and the
re-hashed table (k_repack, k_rehash, cm_build_fast_table) and the probe kernel (cm_probe_lanes<U, PAIR>), each against the
oracle's Index::Construct / kh_get, key by key and exactly, on the crafted references of tests/index_refs.py (at most 15 kb).

Not covered here: tables beyond one re-pack slab (2^24 buckets); references beyond 32-bit coordinates; k_probe_range (its
surplus blocks and ranges: tests/test_gpu_probe_surplus.py)."""
import ctypes as C

import numpy as np
import pytest

import index_refs
import oracle_lib as ol
from chromap_amd import ChromapGPU, _capi

pytestmark = pytest.mark.gpu
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
POISON8, POISON64 = 0xEE, np.uint64(0xEEEEEEEEEEEEEEEE)


# ---- the oracle's side ------------------------------------------------------------------------
class OraBuilt:
    """ora_index_build over a FASTA written from [(name, bytes)]"""
    def __init__(self, seqs, k, w, path):
        self.O = ol.lib()
        self.fa = index_refs.write_fasta(path, seqs)
        self.ref = ol.OraRef()
        assert self.O.ora_ref_load(self.fa.encode(), C.byref(self.ref)) == 0
        self.idx = ol.OraIndex()
        assert self.O.ora_index_build(C.byref(self.ref), k, w, C.byref(self.idx)) == 0
        self.n_minimizers = 0
        for r, (_, s) in enumerate(seqs):
            h = np.zeros(len(s) + 1, np.uint64)
            t = np.zeros(len(s) + 1, np.uint64)
            self.n_minimizers += self.O.ora_minimizers(s, len(s), r, k, w, h.ctypes.data, t.ctypes.data)

    def close(self):
        self.O.ora_index_free(C.byref(self.idx))
        self.O.ora_ref_free(C.byref(self.ref))


def ora_arrays(idx):
    """(occupied bool [nb], deleted bool [nb], keys, vals, occ) of an ora_index, copied"""
    nb = idx.n_buckets
    fl = np.ctypeslib.as_array(idx.flags, shape=(max(1, nb >> 4),)).copy()
    i = np.arange(nb, dtype=np.uint32)
    two = (fl[i >> 4] >> ((i & 15) << 1)) & 3
    keys = np.ctypeslib.as_array(idx.keys, shape=(nb,)).copy()
    vals = np.ctypeslib.as_array(idx.vals, shape=(nb,)).copy()
    occ = np.ctypeslib.as_array(idx.occ, shape=(idx.n_occ,)).copy() if idx.n_occ else np.zeros(0, np.uint64)
    return two == 0, (two & 1) != 0, keys, vals, occ


def ora_lookup(O, idx, hashes):
    """kh_get per hash: (kind uint8, value uint64, buckets visited uint64)"""
    nb = idx.n_buckets
    kind = np.zeros(len(hashes), np.uint8)
    val = np.zeros(len(hashes), np.uint64)
    vis = np.zeros(len(hashes), np.uint64)
    for j, h in enumerate(hashes):
        st = C.c_uint64(0)
        i = O.ora_kh_get(C.byref(idx), int(h) << 1, C.byref(st))
        vis[j] = st.value
        if i != nb:
            kind[j] = _capi.PROBE_SINGLETON if idx.keys[i] & 1 else _capi.PROBE_MULTI
            val[j] = idx.vals[i]
    return kind, val, vis


# ---- the device's side ------------------------------------------------------------------------
def export(g):
    """(k, w, n_buckets, n_occ, n_minimizers, n_keys, buckets uint64 [nb, 2], occ)"""
    k, w = C.c_int32(0), C.c_int32(0)
    nb, nocc = C.c_uint32(0), C.c_uint32(0)
    nmm, nkeys = C.c_uint64(0), C.c_uint64(0)
    assert g.L.cmgpu_index_info(g.ctx, C.byref(k), C.byref(w), C.byref(nb), C.byref(nocc), C.byref(nmm), C.byref(nkeys)) == 0
    bk = np.full((nb.value, 2), 0x77, np.uint64)
    occ = np.zeros(max(1, nocc.value), np.uint64)
    assert g.L.cmgpu_export_index(g.ctx, bk.ctypes.data, occ.ctypes.data) == 0
    return k.value, w.value, nb.value, nocc.value, nmm.value, nkeys.value, bk, occ[:nocc.value]


def sorted_pairs(keys, vals):
    o = np.lexsort((vals, keys))
    return keys[o], vals[o]


def ora_from_export(O, e):
    """the device's file-layout table as an ora_index: same bucket indexes, so kh_get's walk is the probe kernel's"""
    idx = ol.OraIndex()
    assert O.ora_index_from_buckets(e[6].ctypes.data, e[2], e[7].ctypes.data if e[3] else None, e[3], e[0], e[1], C.byref(idx)) == 0
    return idx


# ---- a. the device build equals the oracle's index ----------------------------------------------
@pytest.mark.parametrize("k,w", [(17, 7), (16, 7), (22, 10), (21, 11), (28, 32), (15, 5)])
def test_device_build_equals_oracle(k, w, tmp_path):
    seqs = index_refs.edge_reference(k, w)
    ob = OraBuilt(seqs, k, w, str(tmp_path / "edge.fa"))
    g = ChromapGPU(ref_path=ob.fa, build_index=(k, w))
    try:
        gk, gw, nb, nocc, nmm, nkeys, bk, occ = export(g)
        occd, _, okeys, ovals, oocc = ora_arrays(ob.idx)
        assert (gk, gw) == (k, w)
        assert nb == ob.idx.n_buckets
        assert nkeys == ob.idx.n_keys == int(occd.sum())
        assert nmm == ob.n_minimizers
        assert nocc == ob.idx.n_occ and nocc > 0     # the planted unit's keys
        full = bk[:, 0] != EMPTY
        assert int(full.sum()) == nkeys
        # bucket placement may differ (insertion order), the multiset of (key, value) may not
        a, b = sorted_pairs(bk[full, 0], bk[full, 1]), sorted_pairs(okeys[occd], ovals[occd])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(occ, oocc)
        assert np.all(bk[~full, 0] == EMPTY)         # (nothing left of the 0x77 fill either)
        assert len(np.unique(bk[full, 0] >> np.uint64(1))) == nkeys
    finally:
        g.close()
        ob.close()


# ---- b. the saved file --------------------------------------------------------------------------
@pytest.mark.parametrize("k,w", [(17, 7), (16, 7)])
def test_saved_file_read_by_oracle_and_by_the_loader(k, w, tmp_path):
    seqs = index_refs.edge_reference(k, w)
    ob = OraBuilt(seqs, k, w, str(tmp_path / "edge.fa"))
    O = ob.O
    path = str(tmp_path / "device.idx")
    g = ChromapGPU(ref_path=ob.fa, build_index=(k, w))
    try:
        g.save_index(path)
        e = export(g)
    finally:
        g.close()
    ld = ol.OraIndex()
    assert O.ora_index_load(path.encode(), C.byref(ld)) == 0
    try:
        for f in ("k", "w", "n_keys", "n_buckets", "size", "n_occupied", "upper_bound", "n_occ"):
            assert getattr(ld, f) == getattr(ob.idx, f), f
        occd, _, okeys, ovals, oocc = ora_arrays(ob.idx)
        locc, ldel, lkeys, lvals, loccs = ora_arrays(ld)
        assert np.array_equal(loccs, oocc) and not ldel.any()
        # the flags mark exactly the occupied buckets
        assert np.array_equal(locc, e[6][:, 0] != EMPTY)
        for key, val in zip(okeys[occd].tolist(), ovals[occd].tolist()):
            i = O.ora_kh_get(C.byref(ld), key, None)
            assert i != ld.n_buckets and ld.keys[i] == key and ld.vals[i] == val
        have = set((okeys[occd] >> np.uint64(1)).tolist())
        rng = np.random.RandomState(5)
        absent = [h for h in (rng.randint(0, 1 << 62, 1200, dtype=np.int64) & ((1 << (2 * k)) - 1)).tolist() if h not in have][:1000]
        assert len(absent) == 1000
        for h in absent:
            assert O.ora_kh_get(C.byref(ld), h << 1, None) == ld.n_buckets
    finally:
        O.ora_index_free(C.byref(ld))
        ob.close()
    # the same file through the product's loader and cmgpu_create: the same buckets at the same bucket indexes
    g2 = ChromapGPU(path, ob.fa)
    try:
        e2 = export(g2)
        assert e2[:4] == e[:4]
        assert np.array_equal(e2[6], e[6]) and np.array_equal(e2[7], e[7])
    finally:
        g2.close()


# ---- c. sizing at the seams ---------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", sorted(index_refs.TINY_BUCKETS))
def test_bucket_count_at_khash_thresholds(n_keys, tmp_path):
    k, w = index_refs.TINY_K, index_refs.TINY_W
    seqs = index_refs.tiny_reference(index_refs.TINY_LENGTHS[n_keys])
    ob = OraBuilt(seqs, k, w, str(tmp_path / "tiny.fa"))
    g = ChromapGPU(ref_path=ob.fa, build_index=(k, w))
    try:
        assert ob.idx.n_keys == n_keys and ob.idx.n_buckets == index_refs.TINY_BUCKETS[n_keys]
        e = export(g)
        assert e[5] == n_keys and e[2] == ob.idx.n_buckets
        occd, _, okeys, ovals, _ = ora_arrays(ob.idx)
        full = e[6][:, 0] != EMPTY
        a, b = sorted_pairs(e[6][full, 0], e[6][full, 1]), sorted_pairs(okeys[occd], ovals[occd])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        g.close()
        ob.close()


def test_reference_without_a_kmer_is_refused(tmp_path):
    L = _capi.lib()
    k, w = 17, 7
    rv, keep = index_refs.ref_view(index_refs.no_kmer_reference(k))
    p = _capi.default_params(None)
    ctx = C.c_void_p()
    rc = L.cmgpu_create_from_reference(C.byref(rv), k, w, C.byref(p), 0, C.byref(ctx))
    assert rc == -1 and not ctx.value                      # CMGPU_EINVAL
    assert L.cmgpu_last_error_thread() == b"reference has no minimizers"
    # ... and the next create is not affected
    rv2, keep2 = index_refs.ref_view(index_refs.tiny_reference(index_refs.TINY_LENGTHS[3]))
    rc = L.cmgpu_create_from_reference(C.byref(rv2), k, w, C.byref(p), 0, C.byref(ctx))
    assert rc == 0 and ctx.value
    n = C.c_uint64(0)
    assert L.cmgpu_index_info(ctx, None, None, None, None, None, C.byref(n)) == 0 and n.value == 3
    L.cmgpu_destroy(ctx)


# ---- d. re-pack of a loaded file ----------------------------------------------------------------
def test_repack_of_an_oracle_file_and_a_deleted_bucket(tmp_path):
    k, w = 17, 7
    seqs = index_refs.edge_reference(k, w)
    ob = OraBuilt(seqs, k, w, str(tmp_path / "edge.fa"))
    O = ob.O
    try:
        path = str(tmp_path / "oracle.idx")
        assert O.ora_index_save(path.encode(), C.byref(ob.idx)) == 0
        occd, _, okeys, ovals, oocc = ora_arrays(ob.idx)
        g = ChromapGPU(path, ob.fa)
        try:
            e = export(g)
            assert e[2] == ob.idx.n_buckets and e[3] == ob.idx.n_occ
            assert np.array_equal(e[6][:, 0] != EMPTY, occd)
            assert np.array_equal(e[6][occd, 0], okeys[occd]) and np.array_equal(e[6][occd, 1], ovals[occd])
            assert np.all(e[6][~occd, 1] == 0) and np.array_equal(e[7], oocc)
        finally:
            g.close()
        # a key whose walk passes another key's bucket first: delete that bucket
        hashes = okeys[occd] >> np.uint64(1)
        _, _, vis = ora_lookup(O, ob.idx, hashes)
        behind = int(hashes[int(np.argmax(vis))])
        assert vis.max() >= 2
        home = behind & (ob.idx.n_buckets - 1)
        assert occd[home] and int(okeys[home]) >> 1 != behind
        gone = int(okeys[home]) >> 1
        ob.idx.flags[home >> 4] |= 1 << ((home & 15) << 1)   # __ac_set_isdel_true
        path2 = str(tmp_path / "deleted.idx")
        assert O.ora_index_save(path2.encode(), C.byref(ob.idx)) == 0
        want = ora_lookup(O, ob.idx, hashes)
        at = {int(h): j for j, h in enumerate(hashes)}
        assert want[0][at[gone]] == _capi.PROBE_MISS and want[0][at[behind]] != _capi.PROBE_MISS
        assert int((want[0] == _capi.PROBE_MISS).sum()) == 1
        g = ChromapGPU(path2, ob.fa)
        try:
            assert export(g)[6][home, 0] == np.uint64(0xFFFFFFFFFFFFFFFE)   # the deleted mark, at its bucket
            for file_table in (True, False):     # the file layout keeps the deleted bucket in the walk, the re-hashed table drops it
                kind, val, steps, hits = _capi.debug_probe(g.L, g.ctx, hashes, 4, 1, file_table)
                assert np.array_equal(kind, want[0]) and np.array_equal(val, want[1])
                assert hits == len(hashes) - 1
                if file_table:
                    assert steps == int(want[2].sum())
            assert g.get_option("probe_table_buckets") == 2 * ob.idx.n_buckets
        finally:
            g.close()
    finally:
        ob.close()


# ---- e. the probe kernel, per key ---------------------------------------------------------------
class ProbeCase:
    """one context, its file-layout table as the oracle sees it, the hashes and kh_get's answers, computed once"""
    def __init__(self, seqs, k, w, path):
        self.fa = index_refs.write_fasta(path, seqs)
        self.g = ChromapGPU(ref_path=self.fa, build_index=(k, w))
        self.O = ol.lib()
        self.e = export(self.g)
        self.idx = ora_from_export(self.O, self.e)
        nb = self.nb = self.e[2]
        full = self.e[6][:, 0] != EMPTY
        keys = self.e[6][full, 0] >> np.uint64(1)
        have = set(keys.tolist())
        rng = np.random.RandomState(11)
        absent = []
        while len(absent) < len(keys):
            h = int(rng.randint(0, 1 << 62, dtype=np.int64)) & ((1 << (2 * k)) - 1)
            if h not in have:
                absent.append(h)
        # absent hashes that start at chosen buckets: both ends of the table and the homes of the three longest chains
        _, _, vis = ora_lookup(self.O, self.idx, keys)
        homes = [0, 3, nb - 2, nb - 1] + [int(keys[j]) & (nb - 1) for j in np.argsort(vis)[::-1][:3]]
        self.longest = int(vis.max())
        bits = nb.bit_length() - 1
        crafted = []
        for b in homes:
            for _ in range(4):
                while True:
                    h = (int(rng.randint(1, 1 << 20)) << bits) | b
                    if h not in have:
                        break
                crafted.append(h)
        self.n_keys = len(keys)
        hashes = np.array(keys.tolist() + absent + crafted, np.uint64)
        self.hashes = hashes[rng.permutation(len(hashes))]
        self.want = ora_lookup(self.O, self.idx, self.hashes)
        for a in (self.hashes,) + self.want:
            a.setflags(write=False)

    def close(self):
        self.g.close()
        self.O.ora_index_free(C.byref(self.idx))


@pytest.fixture(scope="module")
def probe_cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("probe")
    cases = {"edge": ProbeCase(index_refs.edge_reference(17, 7), 17, 7, str(d / "edge.fa")),
             "four_buckets": ProbeCase(index_refs.tiny_reference(index_refs.TINY_LENGTHS[3]), 17, 7, str(d / "tiny.fa"))}
    yield cases
    for c in cases.values():
        c.close()


VARIANTS = [(u, p) for u in (1, 2, 4, 8) for p in (0, 1)]


@pytest.mark.parametrize("table", ["edge", "four_buckets"])
def test_probe_cases_are_what_they_claim(table, probe_cases):
    c = probe_cases[table]
    kind, val, vis = c.want
    assert int((kind != _capi.PROBE_MISS).sum()) == c.n_keys and int((kind == _capi.PROBE_MISS).sum()) > c.n_keys
    if table == "edge":
        assert c.nb > 8 * 256 and len(c.hashes) > 8 * 256 + 1     # several blocks at every lookups-per-lane
        assert (kind == _capi.PROBE_SINGLETON).any() and (kind == _capi.PROBE_MULTI).any()
        assert c.longest >= 3 and int(vis.max()) >= c.longest
    else:
        assert c.nb == 4 and c.n_keys == 3


@pytest.mark.parametrize("u,pair", VARIANTS)
@pytest.mark.parametrize("table", ["edge", "four_buckets"])
def test_probe_file_table_equals_kh_get(table, u, pair, probe_cases):
    c = probe_cases[table]
    kind, val, steps, hits = _capi.debug_probe(c.g.L, c.g.ctx, c.hashes, u, pair, True)
    assert np.array_equal(kind, c.want[0])
    assert np.array_equal(val, c.want[1])
    assert steps == int(c.want[2].sum())
    assert hits == c.n_keys


@pytest.mark.parametrize("shift", [1, 2, 3, 4])
@pytest.mark.parametrize("table", ["edge", "four_buckets"])
def test_probe_rehashed_table_equals_kh_get(table, shift, probe_cases):
    c = probe_cases[table]
    try:
        c.g.set_option("probe_table_shift", shift)
        assert c.g.get_option("probe_table_buckets") == c.nb << shift
        for u, pair in VARIANTS:
            kind, val, steps, hits = _capi.debug_probe(c.g.L, c.g.ctx, c.hashes, u, pair, False)
            assert np.array_equal(kind, c.want[0]), (u, pair)
            assert np.array_equal(val, c.want[1]), (u, pair)
            assert hits == c.n_keys
            assert len(c.hashes) <= steps        # (placement follows the order of the atomics: the walks' lengths are not compared)
        # the file's table is still there, untouched
        kind, val, steps, _ = _capi.debug_probe(c.g.L, c.g.ctx, c.hashes, 4, 1, True)
        assert np.array_equal(kind, c.want[0]) and np.array_equal(val, c.want[1]) and steps == int(c.want[2].sum())
    finally:
        c.g.set_option("probe_table_shift", 1)
    assert c.g.get_option("probe_table_buckets") == 2 * c.nb


@pytest.mark.parametrize("u,pair", VARIANTS)
def test_probe_short_launches_keep_to_n(u, pair, probe_cases):
    c = probe_cases["edge"]
    slack = 8 * 256 + 256
    for n in sorted({1, 255, 256, 257, u * 256 - 1, u * 256 + 1}):
        for file_table in (True, False):
            kind, val, steps, hits = _capi.debug_probe(c.g.L, c.g.ctx, c.hashes[:n], u, pair, file_table, slack=slack)
            assert np.array_equal(kind[:n], c.want[0][:n]) and np.array_equal(val[:n], c.want[1][:n]), (n, file_table)
            assert np.all(kind[n:] == POISON8) and np.all(val[n:] == POISON64), (n, file_table)
            assert hits == int((c.want[0][:n] != _capi.PROBE_MISS).sum())
            if file_table:
                assert steps == int(c.want[2][:n].sum())
