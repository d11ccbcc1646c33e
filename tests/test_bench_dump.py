"""bench.py --dump-outputs on the host: what it writes for the record layouts a mapping call hands back (BED records,
pairs records, SAM records), with a stand-in for the device context -- float64 arrays, exact values, the 64 MB cap,
the same seeded sample of read ids from run to run."""
import ctypes as C
import os

import numpy as np

import bench
from chromap_amd import _capi


class FakeMapper:
    """download_records / download_sam of a context whose last batch mapped n_pairs pairs, one record each"""

    def __init__(self, n_pairs, split=0, sam=False):
        self.n_pairs = n_pairs
        self.params = _capi.Params()
        self.params.split_alignment = split
        self.params.output_format = _capi.FORMAT_SAM if sam else 0

    def download_records(self, capacity):
        rec = (_capi.Record * max(1, capacity))()
        a = np.frombuffer(rec, dtype=np.dtype(_capi.Record), count=capacity)
        a["read_id"] = np.arange(capacity)
        a["rid"] = np.arange(capacity) % 24
        a["fragment_start"] = 0xfffffff0 - np.arange(capacity)
        return rec, capacity

    def download_sam(self):
        rec = (_capi.SamRecord * (2 * self.n_pairs))()
        a = np.frombuffer(rec, dtype=np.dtype(_capi.SamRecord), count=2 * self.n_pairs)
        a["read_id"] = np.arange(2 * self.n_pairs) // 2
        a["tlen"] = -7
        a["valid"][::4] = 1
        return rec, None, None, 0, 2 * self.n_pairs


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_all_records_when_they_fit(tmp_path):
    bench.dump_outputs(str(tmp_path), FakeMapper(1000), 1000, 1000)
    got = _load(str(tmp_path))
    assert set(got) == {"records_" + f for f, _ in _capi.Record._fields_} | {"records_total"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["records_total"].tolist() == [1000]
    assert got["records_read_id"].tolist() == list(range(1000))
    assert got["records_fragment_start"][0] == 0xfffffff0  # (u32 values stay exact)


def test_seeded_sample_of_a_large_batch(tmp_path):
    n = 4_000_000
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, FakeMapper(n), n, n)
    bench.dump_outputs(b, FakeMapper(n), n, n)
    ga, gb = _load(a), _load(b)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 << 20
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)
    ids = ga["records_read_id"]
    assert 0 < len(ids) < n and np.all(np.diff(ids) > 0)  # a subset, in pair order
    assert ga["records_total"].tolist() == [n]


def test_pairs_and_sam_layouts(tmp_path):
    bench.dump_outputs(str(tmp_path / "p"), FakeMapper(500, split=1), 500, 500)
    assert {"records_pos1", "records_rid2", "records_strand2"} <= set(_load(str(tmp_path / "p")))
    bench.dump_outputs(str(tmp_path / "s"), FakeMapper(500, sam=True), 1000, 500)
    s = _load(str(tmp_path / "s"))
    assert "records_valid" not in s and len(s["records_tlen"]) == 250 and set(s["records_tlen"].tolist()) == {-7.0}
    assert C.sizeof(_capi.SamRecord) == np.dtype(_capi.SamRecord).itemsize
