"""--allocate-multi-mappings on the device (cm_post.hip: the stage between cmgpu_store_format's selection and its line offsets).
The pins are the reference binary's own bytes and counts (tests/golden/alloc); hand-made records check the device against the host
writers and against a brute-force count of the weights, on the edges the fixtures do not reach."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import alloc_lib
import datasets as ds
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CLI = os.path.join(ds.ROOT, "chromap_amd", "chromap-amd")
REF = os.path.join(ds.ROOT, "oracle", "_ref", "chromap")
GEN = os.path.join(ds.ROOT, "tools", "gen_synth.py")
INFO_LINES = (r"Got all (\d+) multi-mappings!", r"Allocated (\d+) multi-mappings in [0-9.]+s\.",
              r"# multi-mappings that have no uni-mapping overlaps: (\d+)\.")


def _first_difference(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i in range(min(len(g), len(w))):
        if g[i] != w[i]:
            return i, g[i], w[i]
    return min(len(g), len(w)), len(g), len(w)


# ---- (a) C ABI: map, store_append_resident, store_format
@pytest.mark.parametrize("case", alloc_lib.CASES)
def test_store_format_equals_reference(case):
    from chromap_amd import ChromapGPU, _capi
    meta = ds.case_meta(case)
    fa, r1, r2 = ds.case_inputs(case)
    preset, kw = alloc_lib.params_of(meta["chromap_flags"])
    g = ChromapGPU(ds.case_index(case), fa, preset=preset, **kw)
    assert g.store_allocation_info() == (0, 0, 0)
    mate = ds.single_end_mate(case)
    if mate:
        b, off = ol.read_fastx(r1 if mate == 1 else r2)
        _, k = g.map_single(b, off)
        kind, bl = _capi.TEXT_BED_SE, 0
    else:
        b1, o1 = ol.read_fastx(r1)
        b2, o2 = ol.read_fastx(r2)
        if ds.has_barcodes(case):
            bcf, wlf = ds.case_barcode_inputs(case)
            bc, bcq, bco = ol.read_fastq_qual(bcf)
            g.set_whitelist_file(wlf, int(bco[1] - bco[0]))
            g.compute_barcode_abundance(bc, bco)
            _, k = g.map_pairs_barcoded(b1, o1, b2, o2, bc, bcq, bco)
            kind, bl = _capi.TEXT_BED_PE_BC, g.barcode_length
        else:
            _, k = g.map_pairs(b1, o1, b2, o2)
            kind, bl = _capi.TEXT_BED_PE, 0
    assert g.store_append_resident() == k
    lines, nbytes = g.store_format(kind, barcode_length=bl)
    got = bytes(g.store_text())
    want = alloc_lib.golden(case)
    assert got == want, _first_difference(got, want)
    assert hashlib.md5(got).hexdigest() == meta["output_md5"]
    assert lines == meta["reference_stderr_counters"]["num_output"] and nbytes == len(want)
    assert g.store_allocation_info() == alloc_lib.counts(meta)
    # the flag off, and the flag in low-memory mode: the plain texts, and no counts
    p = _capi.default_params(preset, **dict(kw, allocate_multi_mappings=0))
    g.store_format(kind, params=p, barcode_length=bl)
    assert hashlib.md5(bytes(g.store_text())).hexdigest() == meta["plain_md5"]
    assert g.store_allocation_info() == (0, 0, 0)
    if not (ds.has_barcodes(case) and "--remove-pcr-duplicates" in meta["chromap_flags"]):  # (bulk-level removal there: the CLI test's)
        p = _capi.default_params(preset, **dict(kw, low_memory_mode=1))
        g.store_format(kind, params=p, barcode_length=bl)
        assert hashlib.md5(bytes(g.store_text())).hexdigest() == meta["low_mem_md5"]
        assert g.store_allocation_info() == (0, 0, 0)
    g.close()


# ---- (b) command line, FASTQ files through the device ingest
def _amd_index(case):
    fa, _, _ = ds.case_inputs(case)
    idx = os.path.join(ds.CACHE, "amd_" + ds.case_meta(case)["input_md5"]["fa"][:12] + ".idx")
    if not os.path.exists(idx):
        subprocess.run([CLI, "-i", "-r", fa, "-o", idx + ".tmp"], check=True, stderr=subprocess.PIPE)
        os.replace(idx + ".tmp", idx)
    return idx


def _run_cli(case, out, extra=()):
    meta = ds.case_meta(case)
    fa, r1, r2 = ds.case_inputs(case)
    mate = ds.single_end_mate(case)
    reads = ["-1", r1 if mate == 1 else r2] if mate else ["-1", r1, "-2", r2]
    if ds.has_barcodes(case):
        bcf, wlf = ds.case_barcode_inputs(case)
        reads += ["-b", bcf, "--barcode-whitelist", wlf]
    r = subprocess.run([CLI] + meta["chromap_flags"] + list(extra) + ["-x", _amd_index(case), "-r", fa] + reads + ["-o", out], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    with open(out, "rb") as f:
        return f.read(), r.stderr.decode()


@pytest.mark.parametrize("case", alloc_lib.CASES)
def test_cli_equals_reference(case, tmp_path):
    meta = ds.case_meta(case)
    got, err = _run_cli(case, str(tmp_path / "out.bed"))
    want = alloc_lib.golden(case)
    assert got == want, _first_difference(got, want)
    for pat, n in zip(INFO_LINES, alloc_lib.counts(meta)):
        m = re.search(pat, err)
        assert m and int(m.group(1)) == n, (pat, err[-1500:])


@pytest.mark.parametrize("case", ["alloc/al1_pe_n5_q0", "alloc/al6_pe_bc_n3_dedup_q0"])
def test_cli_low_mem_allocates_nothing(case, tmp_path):
    meta = ds.case_meta(case)
    got, err = _run_cli(case, str(tmp_path / "out.bed"), ["--low-mem"])
    assert hashlib.md5(got).hexdigest() == meta["low_mem_md5"]
    assert "does nothing in low-memory mode" in err and "Got all" not in err


# ---- (c) device against host writer and against a brute-force model, on hand-made records
N_SEQ = 6   # chr0: no records; chr1: multi-mappings only; chr2: uni-mappings only; chr3, chr4, chr5: both
BIG = 3000  # members of the largest read: many blocks of the weight kernel and of the scan by key


def _raw(start, end, direction, kind, tn5):
    """(fragment_start, fragment_length) of a record whose coordinates AFTER the in-memory Tn5 shift are [start, end)"""
    if not tn5:
        return start, end - start
    if kind == 1:
        return (start - 4, end - start) if direction == 1 else (start, end - start + 5)
    return start - 4, end - start + 9


def _records(kind, tn5, distance, dup_frac, seed):
    """A few thousand records built for the edges (coordinates given after the shift); (rid, start) is unique per run of duplicates,
    so a text line identifies its record"""
    from chromap_amd.distributed import REC_DTYPE
    rng = np.random.default_rng(seed)
    rows = []  # (read_id, rid, start, end, mapq, direction)
    used = {r: set() for r in range(N_SEQ)}

    def place(rid, lo=1000, hi=400000):
        while True:
            s = int(rng.integers(lo, hi))
            if s not in used[rid]:
                used[rid].add(s)
                return s
    next_read = [0]

    def read():
        next_read[0] += 1
        return next_read[0] * 3 + 1  # (ids with gaps, not in position order)
    # uni-mappings: MAPQ 4 is the lowest
    for rid, cnt in ((2, 700), (3, 900), (4, 900), (5, 500)):
        for _ in range(cnt):
            s = place(rid)
            rows.append((read(), rid, s, s + int(rng.integers(40, 400)), int(rng.choice([4, 4, 5, 30, 60])), int(rng.integers(0, 2))))
    # multi-mappings, MAPQ 0..3: reads of 1..5 members on chr1, chr3, chr4, chr5
    for _ in range(500):
        rd, m = read(), int(rng.integers(1, 6))
        for _ in range(m):
            rid = int(rng.choice([1, 3, 4, 5]))
            s = place(rid)
            rows.append((rd, rid, s, s + int(rng.integers(40, 400)), int(rng.choice([0, 1, 2, 3, 3])), int(rng.integers(0, 2))))
    # a read of two members, one of BIG, one on three chromosomes
    for m, rids in ((2, [3, 4]), (BIG, [1, 3, 4, 5]), (3, [3, 4, 5])):
        rd = read()
        for t in range(m):
            rid = rids[t % len(rids)]
            s = place(rid)
            rows.append((rd, rid, s, s + int(rng.integers(40, 400)), int(rng.integers(0, 4)), int(rng.integers(0, 2))))
    # edges, away from everything else (positions above 500000).  q: [qs, qe) = [start - d, end + d)
    d = distance
    base = 600000 + 4 * d
    for i, (touch_left, touch_right) in enumerate(((0, 0), (1, 0), (0, 1))):
        s, e = base + i * (20000 + 8 * d), base + i * (20000 + 8 * d) + 100
        rows.append((read(), 4, s, e, 3, 1))                                       # the query: a one-member read
        rows.append((read(), 4, s - d - 90, s - d + touch_left, 4, 1))             # ends at qs (not counted), or one base later
        rows.append((read(), 4, e + d - touch_right, e + d + 150, 4, 0))           # starts at qe (not counted), or one base earlier
    # the clamp: a multi-mapping whose start is below the distance, a uni-mapping in front of it
    rows.append((read(), 5, 25, 125, 2, 1))
    rows.append((read(), 5, 8, 20, 60, 1))
    # MAPQ 3 and 4 side by side at neighbouring positions
    for i in range(20):
        s = 450000 + 700 * i
        rows.append((read(), 3, s, s + 200, 3, 1))
        rows.append((read(), 3, s + 10, s + 210, 4, 0))
    # duplicates: copies of a share of the records under new reads, with any MAPQ (a run may hold multi- and uni-mappings)
    for i in rng.choice(len(rows), int(len(rows) * dup_frac), replace=False):
        _, rid, s, e, _, dr = rows[i]
        rows.append((read(), rid, s, e, int(rng.choice([0, 3, 4, 30])), dr))
    rec = np.zeros(len(rows), REC_DTYPE)
    for i, (rd, rid, s, e, q, dr) in enumerate(rows):
        rs, rl = _raw(s, e, dr, kind, tn5)
        rec[i] = (rd, rid, rs, rl, q, dr, 1 if q >= 4 else 0, 1, min(rl, 60), min(rl, 60), 0)
    rec = rec[rng.permutation(len(rec))]
    if kind != 2:
        return rec
    rb = np.zeros(len(rec), np.dtype([("r", REC_DTYPE), ("barcode", "<u8")]))
    rb["r"] = rec
    rb["barcode"] = rng.integers(0, 3, len(rec)).astype(np.uint64) * np.uint64(0x1234567)
    return rb


def _model(rec, tn5, dedup, distance):
    """kind 0 only.  Survivors of duplicate removal in output order as (rid, start, end, mapq, read_id), the brute-force weight of every
    multi-mapping, and the three counts"""
    r = rec.copy()
    start = r["fragment_start"].astype(np.int64) + (4 if tn5 else 0)
    length = r["fragment_length"].astype(np.int64) - (9 if tn5 else 0)
    order = np.lexsort((r["read_id"], r["is_unique"], r["direction"], r["mapq"], length, start, r["rid"]))
    rid, start, length, mapq, read_id = r["rid"][order], start[order], length[order], r["mapq"][order].astype(int), r["read_id"][order]
    keep = np.ones(len(order), bool)
    if dedup:  # the last record of a run of equal (rid, start, length) survives
        same_next = (rid[:-1] == rid[1:]) & (start[:-1] == start[1:]) & (length[:-1] == length[1:])
        keep[:-1] = ~same_next
    rid, start, end, mapq, read_id = rid[keep], start[keep], (start + length)[keep], mapq[keep], read_id[keep]
    uni = mapq >= 4
    weight = np.zeros(len(rid), np.int64)
    for i in np.nonzero(~uni)[0]:
        qs, qe = max(int(start[i]) - distance, 0), int(end[i]) + distance
        weight[i] = np.count_nonzero(uni & (rid == rid[i]) & (start < qe) & (end > qs))
    sums = {}
    for i in np.nonzero(~uni)[0]:
        sums[int(read_id[i])] = sums.get(int(read_id[i]), 0) + int(weight[i])
    counts = (int(np.count_nonzero(~uni)), sum(1 for v in sums.values() if v > 0), sum(1 for v in sums.values() if v == 0))
    return rid, start, end, mapq, read_id, weight, sums, counts


@pytest.fixture(scope="module")
def gpu():
    from chromap_amd import ChromapGPU
    fa, _, _ = ds.case_inputs("toy_chip")
    g = ChromapGPU(ds.case_index("toy_chip"), fa, preset="chip")
    g.names = [b"chr%d" % i for i in range(N_SEQ)]
    g.barcode_length = 16
    yield g
    g.close()


def _format(g, rec, kind, p):
    g.store_clear()
    g.store_append(rec.ctypes.data, len(rec), barcoded=kind in (2, 4, 5, 6))
    lines, nbytes = g.store_format(kind, params=p, barcode_length=16 if kind in (2, 4, 5, 6) else 0)
    text = bytes(g.store_text())
    assert len(text) == nbytes and text.count(b"\n") == lines * (2 if kind in (3, 4) else 1)
    return text, g.store_allocation_info()


@pytest.mark.parametrize("kind,dedup,tn5,q,distance,seed", [
    (0, 0, 0, 0, 0, 11), (0, 1, 0, 2, 200, 11), (0, 1, 1, 30, 1000, 7), (0, 0, 1, 0, 50, 3), (0, 1, 0, 0, 0, 11),
    (1, 0, 0, 0, 0, 11), (1, 1, 1, 2, 200, 7), (1, 0, 1, 30, 1000, 11),
    (2, 1, 0, 0, 200, 11), (2, 0, 1, 2, 0, 5), (2, 1, 1, 30, 1000, 11)])
def test_device_equals_host_writer_and_brute_force(gpu, kind, dedup, tn5, q, distance, seed, tmp_path):
    from chromap_amd import _capi
    g = gpu
    p = _capi.default_params(None, remove_pcr_duplicates=dedup, tn5_shift=tn5, mapq_threshold=q, allocate_multi_mappings=1,
                             multi_mapping_allocation_distance=distance, multi_mapping_allocation_seed=seed)
    rec = _records(kind, tn5, distance, 0.08 if dedup else 0.0, 100 * kind + distance + seed)
    assert 4000 < len(rec) < 12000
    host = rec.copy()
    out = str(tmp_path / "h.bed")
    (g.write_bed, g.write_bed_se, g.write_bed_bc)[kind](host.ctypes.data, len(host), out, params=p)
    with open(out, "rb") as f:
        want = f.read()
    got, info = _format(g, rec, kind, p)
    assert got == want, _first_difference(got, want)
    p_off = _capi.default_params(None, remove_pcr_duplicates=dedup, tn5_shift=tn5, mapq_threshold=q)
    plain, info_off = _format(g, rec, kind, p_off)
    assert info_off == (0, 0, 0) and info[0] > BIG and info[1] > 100
    it = iter(plain.split(b"\n"))
    assert all(any(ln == pl for pl in it) for ln in got.split(b"\n")), "not a subsequence of the plain text"
    assert len(got) < len(plain) or q >= 4
    # another seed: another text at -q 0 (draws happen), the same counts
    if q == 0:
        p2 = _capi.default_params(None, remove_pcr_duplicates=dedup, tn5_shift=tn5, mapq_threshold=q, allocate_multi_mappings=1,
                                  multi_mapping_allocation_distance=distance, multi_mapping_allocation_seed=seed + 1)
        other, info2 = _format(g, rec, kind, p2)
        assert other != got and info2 == info
    if kind != 0:
        return
    # ---- properties that do not depend on the generator
    rid, start, end, mapq, read_id, weight, sums, counts = _model(rec, tn5, dedup, distance)
    assert info == counts
    assert counts[2] >= 1  # (the edge query that nothing touches, at least)
    where = {(int(rid[i]), int(start[i])): i for i in range(len(rid))}
    assert len(where) == len(rid)
    seen = {}
    printed = np.zeros(len(rid), bool)
    for ln in got.split(b"\n")[:-1]:
        f = ln.split(b"\t")
        i = where[(int(f[0][3:]), int(f[1]))]
        assert int(f[2]) == end[i] and int(f[4]) == mapq[i] and not printed[i]
        printed[i] = True
        if mapq[i] < 4:
            seen[int(read_id[i])] = seen.get(int(read_id[i]), 0) + 1
            assert weight[i] > 0, "the kept member has no uni-mapping around it"
    assert np.all(printed[(mapq >= 4) & (mapq >= q)]), "a uni-mapping that passes -q is missing"
    assert not np.any(printed[mapq < q])
    for rd, s in sums.items():
        members = np.nonzero((read_id == rd) & (mapq < 4))[0]
        if s == 0:
            assert rd not in seen
        elif np.all(mapq[members] >= q):
            assert seen.get(rd, 0) == 1, rd
        else:
            assert seen.get(rd, 0) <= 1, rd
    # the edges were there: a uni-mapping ending exactly at an interval's start, one starting exactly at its end
    multi = np.nonzero(mapq < 4)[0]
    uni_end = {(int(rid[i]), int(end[i])) for i in np.nonzero(mapq >= 4)[0]}
    uni_start = {(int(rid[i]), int(start[i])) for i in np.nonzero(mapq >= 4)[0]}
    assert any((int(rid[i]), max(int(start[i]) - distance, 0)) in uni_end for i in multi)
    assert any((int(rid[i]), int(end[i]) + distance) in uni_start for i in multi)
    assert distance == 0 or any(int(start[i]) < distance for i in multi)


@pytest.mark.parametrize("kind,twin", [(3, 0), (4, 2), (5, None), (6, None)])
def test_tagalign_and_single_end_barcoded_kinds(gpu, kind, twin):
    """the kinds without a host writer: two TagAlign lines per BED line of the same records, the same counts; the single-end
    single-cell kinds drop lines of the plain text and add none"""
    from chromap_amd import _capi
    g = gpu
    p = _capi.default_params(None, remove_pcr_duplicates=1, mapq_threshold=0, allocate_multi_mappings=1, multi_mapping_allocation_distance=200)
    rec = _records(2 if kind in (4, 5, 6) else 0, 0, 200, 0.08, 77)
    got, info = _format(g, rec, kind, p)
    assert info[0] > BIG and info[1] > 100
    if twin is not None:
        bed, info_bed = _format(g, rec, twin, p)
        assert info == info_bed and got.count(b"\n") == 2 * bed.count(b"\n")
        ta = [int(ln.split(b"\t")[1]) for ln in got.split(b"\n")[:-1]]  # (the fragment starts where the earlier of its two reads does)
        assert [min(a, b) for a, b in zip(ta[0::2], ta[1::2])] == [int(ln.split(b"\t")[1]) for ln in bed.split(b"\n")[:-1]]
    plain, _ = _format(g, rec, kind, _capi.default_params(None, remove_pcr_duplicates=1, mapq_threshold=0))
    it = iter(plain.split(b"\n"))
    assert all(any(ln == pl for pl in it) for ln in got.split(b"\n")) and len(got) < len(plain)


def test_store_without_multi_mappings_and_with_nothing_else(gpu):
    from chromap_amd import _capi
    g = gpu
    rec = _records(0, 0, 0, 0.0, 5)
    p = _capi.default_params(None, mapq_threshold=0, allocate_multi_mappings=1)
    p_off = _capi.default_params(None, mapq_threshold=0)
    uni = rec[rec["mapq"] >= 4].copy()
    got, info = _format(g, uni, 0, p)
    plain, _ = _format(g, uni, 0, p_off)
    assert got == plain and len(got) > 10000 and info == (0, 0, 0)
    multi = rec[rec["mapq"] < 4].copy()
    got, info = _format(g, multi, 0, p)
    assert got == b"" and info[0] == len(multi) and info[1] == 0 and info[2] == len(set(multi["read_id"].tolist()))


def test_writers_without_the_stage_refuse_the_flag(gpu):
    from chromap_amd import ChromapError, _capi
    p = _capi.default_params(None, allocate_multi_mappings=1)
    with pytest.raises(ChromapError, match="allocate_multi_mappings"):
        gpu.store_format_sam(params=p)


# ---- (d) the reference binary, 100 000 pairs
@pytest.mark.parametrize("paired", [True, False])
def test_output_equals_reference_binary(paired, tmp_path):
    if not os.path.exists(REF):
        pytest.skip("built reference binary not present")
    pre = str(tmp_path / "d")
    subprocess.check_call([sys.executable, GEN, "--out", pre, "--genome", "8000000", "--chroms", "5", "--pairs", "100000", "--readlen", "50",
                           "--seed", "131"], stdout=subprocess.DEVNULL)
    idx = pre + ".idx"
    subprocess.run([CLI, "-i", "-r", pre + ".fa", "-o", idx], check=True, stderr=subprocess.PIPE)
    common = ["-n", "5", "-q", "0", "--allocate-multi-mappings", "--remove-pcr-duplicates", "-x", idx, "-r", pre + ".fa", "-1", pre + "_1.fq"]
    if paired:
        common += ["-2", pre + "_2.fq"]
    r = subprocess.run([REF] + common + ["-o", pre + ".ref.bed", "-t", "16"], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    g = subprocess.run([CLI] + common + ["-o", pre + ".gpu.bed"], stderr=subprocess.PIPE)
    assert g.returncode == 0, g.stderr.decode()[-2000:]
    assert os.path.getsize(pre + ".ref.bed") > 1000000
    assert ds.md5(pre + ".gpu.bed") == ds.md5(pre + ".ref.bed")
    for pat in INFO_LINES:
        assert re.search(pat, r.stderr.decode()).group(1) == re.search(pat, g.stderr.decode()).group(1), pat
