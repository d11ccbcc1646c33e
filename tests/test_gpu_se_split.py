"""Single-end reads with --split-alignment on the device: the C ABI (cmgpu_map_single / cmgpu_map_single_barcoded), the command
line from FASTQ files (device ingest, both SAM routes), the reference binary at a larger size, and a context that changes between
paired-end and single-end split batches, record store included.  The pins are the reference's own bytes (tests/golden/se_split)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest

import datasets as ds
import oracle_lib as ol
import se_split_cases as sc

pytestmark = pytest.mark.gpu
CLI = os.path.join(ds.ROOT, "chromap_amd", "chromap-amd")
REF = os.path.join(ds.ROOT, "oracle", "_ref", "chromap")
GEN = os.path.join(ds.ROOT, "tools", "gen_synth.py")


def _gpu(case):
    from chromap_amd import ChromapGPU
    fa, fq = sc.inputs(case)
    return ChromapGPU(sc.index(case), fa, **sc.params_kw(case)), fq


def _same(case, got):
    want = sc.golden(case)
    assert got == want, sc.first_difference(got, want)
    assert hashlib.md5(got).hexdigest() == sc.meta(case)["output_md5"]


# ---- (a) C ABI
@pytest.mark.parametrize("case", [c for c in sc.CASES if not sc.is_sam(c) and not sc.has_barcodes(c)])
def test_map_single_records_render_to_reference_text(case, tmp_path):
    """ordinary records (single-end bulk TagAlign is the BED line, mapping_writer.cc:44-67)"""
    g, fq = _gpu(case)
    b, off = ol.read_fastx(fq)
    rec, k = g.map_single(b, off)
    out = str(tmp_path / "g.bed")
    lines = g.write_bed_se(rec, k, out)
    _same(case, open(out, "rb").read())
    ref = sc.meta(case)["reference_stderr_counters"]
    assert lines == ref["num_output"]
    s = g.stats.as_dict()
    for key in sc.COUNTERS:
        assert s[key] == ref[key], key
    g.close()


@pytest.mark.parametrize("case", [c for c in sc.CASES if sc.has_barcodes(c)])
def test_map_single_barcoded_text_equals_reference(case):
    from chromap_amd import _capi
    g, fq = _gpu(case)
    bcf, wlf = sc.barcode_inputs(case)
    b, off = ol.read_fastx(fq)
    bc, bcq, bco = ol.read_fastq_qual(bcf)
    g.set_whitelist_file(wlf, int(bco[1] - bco[0]))
    g.compute_barcode_abundance(bc, bco)
    _, k = g.map_single_barcoded(b, off, bc, bcq, bco)
    assert g.store_append_resident() == k
    lines, _ = g.store_format(_capi.TEXT_BED_SE_BC, barcode_length=g.barcode_length)
    _same(case, bytes(g.store_text()))
    ref = sc.meta(case)["reference_stderr_counters"]
    assert lines == ref["num_output"]
    s = g.stats.as_dict()
    for key in sc.BC_COUNTERS:
        assert s[key] == ref[key], key
    g.close()


# ---- (b) command line, device ingest
def _amd_index(case):
    fa, _ = sc.inputs(case)
    idx = os.path.join(ds.CACHE, "amd_" + sc.meta(case)["input_md5"]["fa"][:12] + ".idx")
    if not os.path.exists(idx):
        subprocess.run([CLI, "-i", "-r", fa, "-o", idx + ".tmp"], check=True, stderr=subprocess.PIPE)
        os.replace(idx + ".tmp", idx)
    return idx


def _run_cli(case, out, extra=()):
    fa, fq = sc.inputs(case)
    reads = ["-1", fq]
    if sc.has_barcodes(case):
        bcf, wlf = sc.barcode_inputs(case)
        reads += ["-b", bcf, "--barcode-whitelist", wlf]
    r = subprocess.run([CLI] + sc.flags(case) + list(extra) + ["-x", _amd_index(case), "-r", fa] + reads + ["-o", out], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return open(out, "rb").read()


@pytest.mark.parametrize("case", sc.CASES)
def test_cli_equals_reference_made_golden(case, tmp_path):
    _same(case, _run_cli(case, str(tmp_path / "out.txt")))


@pytest.mark.parametrize("case", [c for c in sc.CASES if sc.is_sam(c)])
def test_cli_sam_host_ingest_route(case, tmp_path):
    """--host-ingest: the host parser and cmgpu_write_sam instead of the reads kept in HBM and the device's SAM text"""
    _same(case, _run_cli(case, str(tmp_path / "out.sam"), ["--host-ingest"]))


def test_cli_single_end_pairs_stays_refused(tmp_path):
    case = sc.CASES[0]
    fa, fq = sc.inputs(case)
    r = subprocess.run([CLI, "--split-alignment", "--pairs", "-x", _amd_index(case), "-r", fa, "-1", fq, "-o", str(tmp_path / "o")], stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"No support for single-end HiC yet!" in r.stderr


# ---- (c) the reference binary, 100 000 reads of 150 bases
def test_output_equals_reference_binary(tmp_path):
    if not os.path.exists(REF):
        pytest.skip("built reference binary not present")
    pre = str(tmp_path / "d")
    subprocess.check_call([sys.executable, GEN, "--out", pre, "--genome", "20000000", "--chroms", "6", "--pairs", "100000", "--readlen", "150",
                           "--frag-min", "300", "--frag-max", "800", "--hic", "--seed", "107", "--indel", "0.002"])
    idx = pre + ".idx"
    subprocess.run([CLI, "-i", "-r", pre + ".fa", "-o", idx], check=True, stderr=subprocess.PIPE)
    common = ["--split-alignment", "-q", "0", "-x", idx, "-r", pre + ".fa", "-1", pre + "_1.fq"]
    r = subprocess.run([REF] + common + ["-o", pre + ".ref.bed", "-t", "16"], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    g = subprocess.run([CLI] + common + ["-o", pre + ".gpu.bed"], stderr=subprocess.PIPE)
    assert g.returncode == 0, g.stderr.decode()[-2000:]
    assert os.path.getsize(pre + ".ref.bed") > 1000000
    assert ds.md5(pre + ".gpu.bed") == ds.md5(pre + ".ref.bed")


# ---- (d) one context, paired and single-end split batches in turn
def test_context_changes_between_paired_and_single_end_split_batches(tmp_path):
    from chromap_amd import ChromapGPU
    case = "ss1_bed_mate1_q0"
    fa, r1, r2 = ds.case_inputs(sc.DIR + "/" + case)
    g = ChromapGPU(sc.index(case), fa, **sc.params_kw(case))
    b1, o1 = ol.read_fastx(r1)
    b2, o2 = ol.read_fastx(r2)
    rec_a, ka = g.map_pairs(b1, o1, b2, o2)  # pairs records (24 bytes each, as the ordinary ones)
    first = C.string_at(C.addressof(rec_a), ka * 24)
    rec_s, ks = g.map_single(b1, off=o1)
    out = str(tmp_path / "s.bed")
    g.write_bed_se(rec_s, ks, out)
    _same(case, open(out, "rb").read())
    rec_b, kb = g.map_pairs(b1, o1, b2, o2)
    assert ka == kb and ka > 10000
    assert C.string_at(C.addressof(rec_b), kb * 24) == first
    g.close()


# ---- (e) the record store keeps the kind of its first append, whatever batch the context mapped last
def test_record_store_kind_is_fixed_by_its_first_append():
    from chromap_amd import ChromapError, ChromapGPU
    case = "ss1_bed_mate1_q0"
    fa, r1, r2 = ds.case_inputs(sc.DIR + "/" + case)
    g = ChromapGPU(sc.index(case), fa, **sc.params_kw(case))
    b1, o1 = ol.read_fastx(r1)
    b2, o2 = ol.read_fastx(r2)
    names = [b"r%d" % i for i in range(len(o1) - 1)]
    # single-end split records in the store, then a paired split batch: the pairs formatter must not read them as pairs records
    _, ks = g.map_single(b1, off=o1)
    assert g.store_append_resident() == ks
    _, kp = g.map_pairs(b1, o1, b2, o2)
    with pytest.raises(ChromapError, match="pairs text needs pairs records"):
        g.store_format_pairs(names)
    with pytest.raises(ChromapError, match="mixes pairs records and ordinary records"):
        g.store_append_resident()
    # pairs records in the store, then a single-end batch: the same pairs text as before it
    g.store_clear()
    assert g.store_append_resident() == kp
    lines, nbytes = g.store_format_pairs(names)
    want = bytes(g.store_text())
    assert lines > 10000 and len(want) == nbytes
    g.map_single(b1, off=o1)
    assert g.store_format_pairs(names) == (lines, nbytes)
    assert bytes(g.store_text()) == want
    with pytest.raises(ChromapError, match="mixes pairs records and ordinary records"):
        g.store_append_resident()
    g.close()
