"""--allocate-multi-mappings on the host: the stage functions (host emulation) map the reads of the bulk fixtures of
tests/golden/alloc, cmgpu_write_bed_pe / _se render the records with the case's parameters, and the bytes must be the reference
binary's.  The same records with low_memory_mode = 1 must render to the text of a run without the flag: the reference allocates in
its in-memory flavour only."""
import ctypes as C
import functools
import hashlib

import pytest

import alloc_lib
import datasets
import hostemu_lib as he
import oracle_lib as ol


@functools.lru_cache(maxsize=None)  # (mapped once per case; the renderings work on copies)
def _map(case):
    meta = datasets.case_meta(case)
    fa, r1, r2 = datasets.case_inputs(case)
    preset, kw = alloc_lib.params_of(meta["chromap_flags"])
    h = he.HostEmu(datasets.case_index(case), fa, he.params(preset, **kw))
    mate = datasets.single_end_mate(case)
    if mate:
        b, off = ol.read_fastx(r1 if mate == 1 else r2)
        rec, k, _ = h.map_single(b, off)
    else:
        b1, o1 = ol.read_fastx(r1)
        b2, o2 = ol.read_fastx(r2)
        rec, k, _, _ = h.map_pairs(b1, o1, b2, o2)
    return meta, h, rec, k, mate


def _render(h, rec, k, mate, path, **overrides):
    """the writers sort (and shift) the records in place: every rendering gets its own copy"""
    copy = type(rec)()
    C.memmove(copy, rec, C.sizeof(rec))
    saved = {n: getattr(h.p, n) for n in overrides}
    for n, v in overrides.items():
        setattr(h.p, n, v)
    try:
        lines = (h.write_bed_se if mate else h.write_bed)(copy, k, path)
    finally:
        for n, v in saved.items():
            setattr(h.p, n, v)
    with open(path, "rb") as f:
        return lines, f.read()


@pytest.mark.parametrize("case", alloc_lib.BULK_CASES)
def test_host_writer_matches_reference(case, tmp_path):
    meta, h, rec, k, mate = _map(case)
    assert h.p.allocate_multi_mappings == 1
    lines, got = _render(h, rec, k, mate, str(tmp_path / "a.bed"))
    want = alloc_lib.golden(case)
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        for i in range(min(len(g), len(w))):
            assert g[i] == w[i], (i, g[i], w[i])
    assert hashlib.md5(got).hexdigest() == meta["output_md5"]
    assert lines == meta["reference_stderr_counters"]["num_output"]
    # the flag off: the run without allocation
    _, plain = _render(h, rec, k, mate, str(tmp_path / "p.bed"), allocate_multi_mappings=0)
    assert hashlib.md5(plain).hexdigest() == meta["plain_md5"]
    assert (plain != got) == (meta["plain_md5"] != meta["output_md5"])
    # every allocated line is a plain line, in the same order
    it = iter(plain.split(b"\n"))
    assert all(any(ln == p for p in it) for ln in got.split(b"\n"))


@pytest.mark.parametrize("case", alloc_lib.BULK_CASES)
def test_low_memory_mode_allocates_nothing(case, tmp_path):
    meta, h, rec, k, mate = _map(case)
    _, with_flag = _render(h, rec, k, mate, str(tmp_path / "a.bed"), low_memory_mode=1)
    _, without = _render(h, rec, k, mate, str(tmp_path / "p.bed"), low_memory_mode=1, allocate_multi_mappings=0)
    assert with_flag == without
    assert hashlib.md5(with_flag).hexdigest() == meta["low_mem_md5"]


def test_parameter_defaults():
    p = he.params()
    assert (p.allocate_multi_mappings, p.multi_mapping_allocation_distance, p.multi_mapping_allocation_seed) == (0, 0, 11)
    for preset in ("atac", "chip", "hic"):
        q = he.params(preset)
        assert (q.allocate_multi_mappings, q.multi_mapping_allocation_distance, q.multi_mapping_allocation_seed) == (0, 0, 11)
        assert q.bc_probability_threshold == 0.9


def test_writers_without_the_stage_refuse_the_flag(tmp_path):
    """pairs and SAM records have no allocation stage: their host writers return an error instead of ignoring the flag, and open nothing"""
    L = he.lib()
    p = he.params(allocate_multi_mappings=1)
    out = tmp_path / "x.pairs"
    names = (C.c_char_p * 1)(b"chr1")
    lens = (C.c_uint32 * 1)(1000)
    rn = (C.c_char_p * 1)(b"r")
    assert L.cmgpu_write_pairs_ranked(names, lens, 1, C.byref(p), None, 0, rn, 0, None, str(out).encode()) < 0
    assert not out.exists()
