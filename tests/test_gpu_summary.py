"""--summary on the GPU: every fixture of tests/golden/summary/ (the reference's own CSV, made where its minimizer cache never
answered a read) through chromap-amd on both ingest routes -- the summary must be the fixture's bytes and the BED / pairs / SAM
file of the same run the reference's -- then the multi-GPU path, and the C ABI in several small batches."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import datasets as ds
import oracle_lib as ol
import summary_fixtures as sf

pytestmark = pytest.mark.gpu
CLI = os.path.join(ds.ROOT, "chromap_amd", "chromap-amd")


def _run(name, tmp_path, more=()):
    m = sf.meta(name)
    fa, reads, extra = sf.inputs(name)
    out, csv = str(tmp_path / "out.txt"), str(tmp_path / "summary.csv")
    r = subprocess.run([CLI] + m["chromap_flags"] + extra + ["-x", ds.case_index(m["base_case"]), "-r", fa] + reads +
                       ["-o", out, "--summary", csv] + list(more), stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert b"not computed" in r.stderr  # the one line about the four cache columns
    return m, open(out, "rb").read(), open(csv, "rb").read()


def _check(name, m, out, csv):
    want = sf.csv(name)
    assert hashlib.md5(want).hexdigest() == m["summary_md5"]
    assert csv == want, "summary differs from the reference's:\n" + "\n".join(
        "%s | %s" % (a, b) for a, b in zip(csv.decode().splitlines(), want.decode().splitlines()) if a != b)[:2000]
    assert hashlib.md5(out).hexdigest() == m["output_md5"]
    if m["golden_output"]:
        assert out == ds.case_golden_bed(m["golden_output"])


def test_there_are_fixtures():
    assert len(sf.CASES) >= 12


@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("name", sf.CASES)
def test_summary_equals_reference(name, route, tmp_path):
    m, out, csv = _run(name, tmp_path, ["--host-ingest"] if route == "host" else [])
    _check(name, m, out, csv)


@pytest.mark.parametrize("name", ["b1_atac_bc", "b3_bulk_level_bc_q0"])
def test_summary_through_the_exchange(name, tmp_path):
    m, out, csv = _run(name, tmp_path, ["--force-exchange"])
    _check(name, m, out, csv)


def test_run_without_summary_is_untouched(tmp_path):
    """the same command without --summary: same output, no summary file, no word about it"""
    m = sf.meta("b1_atac_bc")
    fa, reads, extra = sf.inputs("b1_atac_bc")
    out = str(tmp_path / "out.bed")
    r = subprocess.run([CLI] + m["chromap_flags"] + extra + ["-x", ds.case_index(m["base_case"]), "-r", fa] + reads + ["-o", out],
                       stderr=subprocess.PIPE, cwd=str(tmp_path))
    assert r.returncode == 0 and b"Summary" not in r.stderr
    assert open(out, "rb").read() == ds.case_golden_bed("b1_atac_bc")
    assert os.listdir(str(tmp_path)) == ["out.bed"]


def _slice(b, o, lo, hi):
    return np.ascontiguousarray(b[int(o[lo]):int(o[hi])]), np.ascontiguousarray(o[lo:hi + 1] - o[lo])


@pytest.mark.parametrize("name", ["b1_atac_bc", "b1_atac_bc_nowl"])
def test_c_abi_in_small_batches(name, tmp_path):
    """batches of 5000 pairs (the scope of the multi-mapper sampling, so the records are the one-batch run's): keys first appear in
    different batches, the table is read back between them, and the CSV is still the reference's"""
    from chromap_amd import ChromapGPU, _capi
    m = sf.meta(name)
    fa, r1, r2 = ds.case_inputs(m["base_case"])
    bcf, wlf = ds.case_barcode_inputs(m["base_case"])
    preset, kw = ds.flags_to_params(m["chromap_flags"])
    g = ChromapGPU(ds.case_index(m["base_case"]), fa, preset=preset, **kw)
    b1, o1 = ol.read_fastx(r1)
    b2, o2 = ol.read_fastx(r2)
    bc, bcq, bco = ol.read_fastq_qual(bcf)
    bl = int(bco[1] - bco[0])
    if m["barcodes"] == "wl":
        g.set_whitelist_file(wlf, bl)
        g.compute_barcode_abundance(bc, bco)
    g.summary_enable()
    n, seen, total = len(o1) - 1, 0, 0
    for lo in range(0, n, 5000):
        hi = min(n, lo + 5000)
        sb1, so1 = _slice(b1, o1, lo, hi)
        sb2, so2 = _slice(b2, o2, lo, hi)
        sbc, sbo = _slice(bc, bco, lo, hi)
        sbq, _ = _slice(bcq, bco, lo, hi)
        g.map_pairs_barcoded(sb1, so1, sb2, so2, sbc, sbq, sbo, first_read_id=lo)
        g.store_append_resident()
        entries, nonwl = g.summary_table()
        assert len(entries) >= seen and all(e[1] < hi for e in entries)
        seen = len(entries)
        total = sum(e[2] for e in entries) + nonwl
        assert total == hi  # every read of the batches so far is counted once
    assert g.summary_info()[0] == seen
    g.store_format(_capi.TEXT_BED_PE_BC, barcode_length=bl)
    csv = str(tmp_path / "s.csv")
    g.write_summary(csv, barcode_length=bl, nonwhitelist_row=m["barcodes"] == "wl")
    assert open(csv, "rb").read() == sf.csv(name)
    assert hashlib.md5(g.store_text()).hexdigest() == m["output_md5"]
    g.summary_clear()
    assert g.summary_table() == ([], 0)
    g.close()
