"""--summary without a GPU: the host CSV writer (cmgpu_write_summary through chromap_amd._capi) fed with tables built here from a
fixture must give the fixture's bytes -- the reference's khash row order, its formats, the paired-end SAM halving, the optional
last column and the non-whitelist row -- and the CLI refuses what it cannot do with a message."""
import os
import subprocess

import pytest

import datasets as ds
import oracle_lib as ol
import summary_fixtures as sf
from chromap_amd import _capi

CLI = os.path.join(ds.ROOT, "chromap_amd", "chromap-amd")


def _table_in_read_order(name, scale=1, odd=0):
    """the fixture's counts keyed by barcode, the keys in the order the reads bring them (no whitelist: the barcode as read).
    scale / odd: dup, lowmapq and mapped as a paired-end SAM run accumulates them before the halving (2x, or 2x + 1)"""
    m = sf.meta(name)
    assert m["barcodes"] == "nowl"
    bc_path, _ = ds.case_barcode_inputs(m["base_case"])
    bases, off = ol.read_fastx(bc_path)
    raw = bytes(bases)
    counts = {sf.key_of(b): (t, d, t - u, lq) for b, t, d, u, lq in sf.rows(name)}
    entries, seen = [], set()
    for i in range(len(off) - 1):
        k = sf.key_of(raw[int(off[i]):int(off[i + 1])].decode())
        if k in seen:
            continue
        seen.add(k)
        t, d, mp, lq = counts[k]
        entries.append((k, i, t, d * scale + odd * (d > 0), lq * scale + odd * (lq > 0), mp * scale + odd * (mp > 0)))
    assert len(entries) == len(counts)
    return entries


def test_there_are_fixtures():
    assert len(sf.CASES) >= 12
    for name in sf.CASES:  # the condition under which the whole file is reproducible: the reference's cache never answered
        assert all(ln.split(",")[5] == "0" for ln in sf.csv(name).decode().splitlines()[1:]), name


def test_khash_order_and_formats(tmp_path):
    out = str(tmp_path / "s.csv")
    entries = _table_in_read_order("b1_atac_bc_nowl")
    assert len(entries) > 400  # enough keys for several doublings of the reference's map
    _capi.write_summary([(entries, 0)], out, barcode_length=16)
    assert open(out, "rb").read() == sf.csv("b1_atac_bc_nowl")


def test_tables_of_several_contexts_and_entry_order(tmp_path):
    """entries in any order, split over two tables with a key in both: counters add up, the smallest first read id stands"""
    out = str(tmp_path / "s.csv")
    entries = _table_in_read_order("b1_atac_bc_nowl")
    k, first, t, d, lq, mp = entries[3]
    a = list(reversed(entries[:200])) + [(k, first + 7, 0, 0, 0, 0)]
    a[a.index(entries[3])] = (k, first, t - 1, d, 0, mp)
    b = entries[200:][::2] + entries[200:][1::2] + [(k, 2 ** 64 - 1, 1, 0, lq, 0)]
    _capi.write_summary([(a, 0), (b, 0)], out, barcode_length=16)
    assert open(out, "rb").read() == sf.csv("b1_atac_bc_nowl")


def test_last_column_switch(tmp_path):
    out = str(tmp_path / "s.csv")
    _capi.write_summary([(_table_in_read_order("b1_atac_bc_nowl_noslots"), 0)], out, barcode_length=16, num_cache_slots_column=False)
    assert open(out, "rb").read() == sf.csv("b1_atac_bc_nowl_noslots")


@pytest.mark.parametrize("odd", [0, 1])
def test_paired_sam_halving(tmp_path, odd):
    out = str(tmp_path / "s.csv")
    _capi.write_summary([(_table_in_read_order("b1_atac_bc_nowl", scale=2, odd=odd), 0)], out, barcode_length=16, halve_pairs=True)
    assert open(out, "rb").read() == sf.csv("b1_atac_bc_nowl")
    (bc, t, d, u, lq), = sf.rows("s1_chip_sam")  # bulk: one row under key 0, the barcode column empty
    assert bc == ""
    _capi.write_summary([([(0, 0, t, 2 * d + odd, 2 * lq + odd, 2 * (t - u) + odd)], 0)], out, halve_pairs=True)
    assert open(out, "rb").read() == sf.csv("s1_chip_sam")


def test_bulk_row_and_nonwhitelist_row(tmp_path):
    out = str(tmp_path / "s.csv")
    (bc, t, d, u, lq), = sf.rows("b1_bulk_chip")
    _capi.write_summary([([(0, 0, t, d, lq, t - u)], 0)], out)
    assert open(out, "rb").read() == sf.csv("b1_bulk_chip")
    # the non-whitelist row ends the file: total = unmapped, everything else 0
    last = sf.csv("b1_atac_bc").decode().splitlines()[-1]
    assert last.startswith("non-whitelist,")
    n = int(last.split(",")[1])
    _capi.write_summary([([], n)], out, barcode_length=16, nonwhitelist_row=True)
    assert open(out, "rb").read().decode().splitlines()[1:] == [last]


@pytest.mark.parametrize("args,needle", [
    (["--summary"], b"missing value for --summary"),
    (["--summary", "s.csv", "--frip-est-params", "1;2;3"], b"expecting 5 parameters but found 3"),
    (["--summary", "s.csv", "--frip-est-params", "1;2;x;4;5"], b"is not a number"),
    (["--summary", "s.csv", "-n", "2"], b"--summary with -n > 1"),
])
def test_cli_refuses_with_a_message(args, needle, tmp_path):
    base = ["-x", "none.idx", "-r", "none.fa", "-1", "none.fq", "-o", str(tmp_path / "o.bed")]
    r = subprocess.run([CLI] + base + args, stderr=subprocess.PIPE, stdout=subprocess.PIPE, cwd=str(tmp_path))
    assert r.returncode != 0 and needle in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "s.csv"))
