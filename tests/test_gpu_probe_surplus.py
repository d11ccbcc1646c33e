"""k_probe_range's surplus blocks: the grid covers an upper bound of 2 * pairs * (longest read / 4 + 3) minimizers, and a block whose
tile lies behind the range's end stores a zero partial from one lane and leaves.  Here the grid is nearly all surplus: nine pairs in
ten are shorter than --min-read-length and emit nothing.  The sum k_probe_reduce makes of every block's partial (Stats.probe_steps)
must equal what k_probe, whose grid is exact, counts on the same minimizers (cmgpu_probe_bench_variant -- the reference of
tests/test_gpu_exchange.py::test_parked_batches_and_probe_shapes); minimizers, counters and records must equal the oracle's."""
import ctypes as C

import numpy as np
import pytest

import fuzz_data
import oracle_lib as ol
import test_hostemu_fuzz as _fz

pytestmark = pytest.mark.gpu


def test_mostly_surplus_probe_grid(tmp_path):
    from chromap_amd import ChromapGPU, Stats
    rng = np.random.default_rng(5)
    chroms, r1, r2 = fuzz_data.make_case(11, genome=90_000, copies=60, pairs=4000, tandem=False)
    for i in range(len(r1)):
        if i % 10:  # below the atac preset's minimum of 30 bases: the pair is dropped before the minimizers
            n = int(rng.integers(1, 30))
            r1[i], r2[i] = r1[i][:n], r2[i][:int(rng.integers(1, 30))]
    fa = str(tmp_path / "f.fa")
    with open(fa, "wb") as f:
        for i, c in enumerate(chroms):
            f.write(b">c%d\n" % i + c.tobytes() + b"\n")

    def pack(rs):
        off = np.zeros(len(rs) + 1, np.uint32)
        off[1:] = np.cumsum([len(r) for r in rs])
        return np.frombuffer(b"".join(rs), np.uint8).copy(), off
    b1, o1 = pack(r1)
    b2, o2 = pack(r2)
    kw = {"mapq_threshold": 0}
    o = ol.Oracle(None, fa, ol.params("atac", **kw))
    idx = str(tmp_path / "f.idx")
    assert o.L.ora_index_save(idx.encode(), C.byref(o.idx)) == 0
    orec, ok, ost, _ = o.map_pairs(b1, o1, b2, o2)
    od = ost.as_dict()
    o.close()
    assert 0 < ok < len(r1) // 8
    g = ChromapGPU(idx, fa, preset="atac", **kw)
    try:
        for u in (1, 4):  # the default shape and the widest tile per block in use
            g.set_option("probe_lookups_per_lane", u)
            st = Stats()
            g.upload(b1, o1, b2, o2)
            k = g.map_resident(st)
            rec, k2 = g.download_records(len(r1))
            assert k2 == k == ok
            assert _fz._tuples_g(rec, k, False) == _fz._tuples_o(orec, ok, False)
            gst = st.as_dict()
            for key in ("num_minimizers", "num_candidates", "num_mappings", "num_mapped_reads", "num_uniquely_mapped_reads"):
                assert gst[key] == od[key], (u, key)
            # the grid's upper bound against what the range holds: at least four blocks in five are surplus
            assert gst["num_minimizers"] * 5 < 2 * len(r1) * (50 // 4 + 3)
            a, ps, hits = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
            assert g.L.cmgpu_probe_bench_variant(g.ctx, gst["num_minimizers"], 1, u, 0, C.byref(a), C.byref(ps), C.byref(hits)) == 0
            assert ps.value == gst["probe_steps"] > 0, (u, ps.value, gst["probe_steps"])
    finally:
        g.close()
