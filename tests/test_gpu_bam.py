"""--BAM on the GPU: the SAM record store and the read store rendered as BAM alignment records (chromap_amd/csrc/cm_bam.h,
cm_sam_post.hip: k_bam_format) must be the plain-Python encoding (tests/bam_model.py) of the reference's golden SAM text, and under
every duplicate rule and filter that of the SAM text the same stores give; compressed, with the header in front, they are a BAM file
that decodes to the golden text; the tabix indexer refuses them; and chromap-amd --BAM writes that file."""
import gzip
import os
import re
import shutil
import struct
import subprocess

import pytest

import bam_model as bm
import bgzf_texts as bt
import datasets
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")
CASES = ["s1_chip_sam", "s1_se_sam", "b1_bc_sam", "h1_hic_sam", "x2_gaps_sam_q0"]
_want = {}


def _golden(case):
    """(golden SAM text, its header bytes, its record bytes, its lines): encoded once"""
    if case not in _want:
        text = datasets.case_golden_bed(case)
        header, records = bm.encode(text)
        _want[case] = (text, header, records, sum(1 for ln in text.split(b"\n") if ln and not ln.startswith(b"@")))
    return _want[case]


def _fill_stores(case, texts=None):
    """a context whose read store and SAM record store hold the case's run (the ingest of tests/test_gpu_sam_device.py); texts: the
    FASTQ text of the read files, where not the case's own"""
    from chromap_amd import ChromapGPU, Stats
    meta = datasets.case_meta(case)
    fa, r1, r2 = datasets.case_inputs(case)
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    g = ChromapGPU(datasets.case_index(case), fa, preset=preset, **kw)
    try:
        mate = datasets.single_end_mate(case)
        files = [r1 if mate == 1 else r2] if mate else [r1, r2]
        texts = texts or [open(f, "rb").read() for f in files]
        bc_len = 0
        g.fastq_keep_reads(True)
        n = g.fastq_scan(0, texts[0], True)
        if not mate:
            assert g.fastq_scan(1, texts[1], True) == n
        if datasets.has_barcodes(case):
            bcf, wlf = datasets.case_barcode_inputs(case)
            bc, _, bco = ol.read_fastq_qual(bcf)
            bc_len = int(bco[1] - bco[0])
            g.set_whitelist_file(wlf, bc_len)
            g.compute_barcode_abundance(bc, bco)
            assert g.fastq_scan(2, open(bcf, "rb").read(), True) == n
            g.fastq_take(2, n)
        g.fastq_take(0, n)
        if not mate:
            g.fastq_take(1, n)
        g.fastq_commit(n, first_read_id=0, paired=not mate, barcoded=bc_len > 0)
        g.map_resident(Stats())
        g.sam_store_clear()
        assert g.sam_store_append_resident() > 100
    except BaseException:
        g.close()
        raise
    return g, bc_len


@pytest.fixture(scope="module")
def stores():
    made = {}

    def get(case):
        if case not in made:
            made[case] = _fill_stores(case)
        return made[case]
    yield get
    for g, _ in made.values():
        g.close()


def _first_difference(got, want):
    at = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    return "%d and %d bytes, first difference at %d: %r, want %r" % (len(got), len(want), at, got[at:at + 16], want[at:at + 16])


def _header_of(g):
    return b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (nm, ln) for nm, ln in zip(g.names, g.reference_lengths()))


# ---- 1. the library: records equal the model's encoding of the golden text, for every group width
@pytest.mark.parametrize("case", CASES)
def test_records_equal_the_encoding_of_the_golden_sam(case, stores):
    g, bc_len = stores(case)
    _, _, want, lines = _golden(case)
    for group in (8, 16, 64):
        g.set_option("sam_format_group", group)
        n, nbytes = g.store_format_bam(barcode_length=bc_len)
        got = g.store_text()
        assert n == lines and nbytes == len(got), group
        assert got == want, (group, _first_difference(got, want))
    g.set_option("sam_format_group", 8)
    at, starts = 0, set()
    while at < len(got):
        starts.add(at % 4)
        at += 4 + struct.unpack_from("<I", got, at)[0]
    assert at == len(got) and starts == {0, 1, 2, 3}, "records at every offset mod 4"


# ---- 2. duplicate rules and the filter: the encoding of the SAM text the same stores give
@pytest.mark.parametrize("case", CASES)
def test_selection_is_the_sam_writers(case, stores):
    from chromap_amd import _capi
    g, bc_len = stores(case)
    header = _header_of(g)
    seen = set()
    for k, (lowmem, thr) in enumerate(((0, 0), (0, 30), (1, 0), (1, 30))):
        p = _capi.Params.from_buffer_copy(g.params)
        p.remove_pcr_duplicates, p.low_memory_mode, p.mapq_threshold = 1, lowmem, thr
        g.set_option("sam_format_group", (8, 16, 64, 8)[k])
        lines, _ = g.store_format_sam(params=p, barcode_length=bc_len)
        sam = g.store_text()
        want = bm.encode(header + sam)[1]
        n, nbytes = g.store_format_bam(params=p, barcode_length=bc_len)
        got = g.store_text()
        assert (n, nbytes) == (lines, len(want)), (lowmem, thr)
        assert got == want, (lowmem, thr, _first_difference(got, want))
        seen.add(lines)
    g.set_option("sam_format_group", 8)
    assert len(seen) >= 2, "the filter drops records here"


# ---- 3. CB:Z through a translation table
def test_translated_barcodes(stores, tmp_path):
    import test_gpu_barcode_translate as tr
    case = "b1_bc_sam"
    g, bc_len = stores(case)
    _, wlf = datasets.case_barcode_inputs(case)
    table = tr.whitelist_table(wlf, str(tmp_path / "tr.tsv"))
    try:
        for group in (8, 16, 64):
            g.set_option("sam_format_group", group)
            g.set_barcode_translation(table)
            lines, _ = g.store_format_sam(barcode_length=bc_len)
            sam = g.store_text()
            assert b"CB:Z:CELL" in sam
            want = bm.encode(_header_of(g) + sam)[1]
            n, nbytes = g.store_format_bam(barcode_length=bc_len)
            got = g.store_text()
            assert (n, nbytes) == (lines, len(want)) and got == want, (group, _first_difference(got, want))
            assert got.count(b"CBZCELL") == lines
    finally:
        g.set_barcode_translation(None)
        g.set_option("sam_format_group", 8)
    g.store_format_bam(barcode_length=bc_len)
    assert g.store_text() == _golden(case)[2]


# ---- 4. compressed, behind the header: a BAM file; the tabix indexer refuses it
@pytest.mark.parametrize("case", ["s1_chip_sam", "b1_bc_sam"])
def test_header_and_compressed_records_decode_to_the_golden_sam(case, stores, tmp_path):
    from chromap_amd import ChromapError
    g, bc_len = stores(case)
    text, header, records, lines = _golden(case)
    g.store_format_bam(barcode_length=bc_len)
    n_blocks, n_out = g.store_compress_text()
    comp = g.store_bgzf()
    assert n_blocks == (len(records) + bt.SLICE - 1) // bt.SLICE and len(comp) == n_out and n_out < len(records)
    bt.check_bgzf(comp, records)
    path = str(tmp_path / "header.bin")
    g.write_bam_header(path)
    got_header = open(path, "rb").read()
    assert got_header == header
    assert bm.decode(got_header + gzip.decompress(comp)) == bm.normalise(text)
    with pytest.raises(ChromapError, match="holds BAM records"):
        g.bgzf_tabix()
    # SAM text from the same context afterwards is text again: the indexer then reads it, and refuses it as SAM, not as BAM
    g.store_format_sam(barcode_length=bc_len)
    g.store_compress_text()
    with pytest.raises(ChromapError) as e:
        g.bgzf_tabix()
    assert "BAM" not in str(e.value)


# ---- 5. a read name that does not fit l_read_name
def _renamed(text, length):
    lines = text.split(b"\n")
    for i in range(0, len(lines) - 3, 4):
        assert lines[i].startswith(b"@")
        lines[i] = b"@" + (b"%07d" % (i // 4)).rjust(length, b"n")
    return b"\n".join(lines)


def test_read_names_of_254_and_255_bytes():
    from chromap_amd import ChromapError
    case = "s1_se_sam"
    _, r1, r2 = datasets.case_inputs(case)
    src = open(r1 if datasets.single_end_mate(case) == 1 else r2, "rb").read()
    g, _ = _fill_stores(case, [_renamed(src, 254)])
    try:
        lines, _ = g.store_format_sam()
        sam = g.store_text()
        n, _ = g.store_format_bam()
        got = g.store_text()
        assert n == lines and got == bm.encode(_header_of(g) + sam)[1]
        assert all(len(ln.split(b"\t")[0]) == 254 for ln in sam.split(b"\n") if ln)
    finally:
        g.close()
    g, _ = _fill_stores(case, [_renamed(src, 255)])
    try:
        with pytest.raises(ChromapError, match="more than 254 bytes"):
            g.store_format_bam()
        assert g.store_text() == b"", "no output"
        assert g.store_format_sam()[0] == lines, "SAM text has no such limit"
    finally:
        g.close()


# ---- 6. the command line
def _cli_args(case):
    fa, r1, r2 = datasets.case_inputs(case)
    m = datasets.single_end_mate(case)
    reads = ["-1", r1, "-2", r2] if not m else ["-1", r1 if m == 1 else r2]
    if datasets.has_barcodes(case):
        bc, wl = datasets.case_barcode_inputs(case)
        reads += ["-b", bc, "--barcode-whitelist", wl]
    return list(datasets.case_meta(case)["chromap_flags"]) + ["-x", datasets.case_index(case), "-r", fa] + reads


def _check_bam_file(raw, case):
    text = _golden(case)[0]
    assert raw.endswith(bt.EOF_BLOCK) and raw.count(bt.EOF_BLOCK) == 1
    for at, size in bt.blocks(raw):
        assert size <= 65536
    assert bm.decode(gzip.decompress(raw)) == bm.normalise(text)


@pytest.mark.parametrize("case,extra", [("s1_chip_sam", []), ("b1_bc_sam", ["--output-bgzf"])])
def test_cli_bam(case, extra, tmp_path):
    out = str(tmp_path / "out.bam")
    r = subprocess.run([CLI] + _cli_args(case) + ["--BAM"] + extra + ["-o", out], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    raw = open(out, "rb").read()
    _check_bam_file(raw, case)
    _, header, records, lines = _golden(case)
    m = re.search(rb"Compressed (\d+) bytes of BAM header and records into (\d+) bytes of BGZF on the device in [0-9.]+s", r.stderr)
    assert m and (int(m.group(1)), int(m.group(2))) == (len(header) + len(records), len(raw)), r.stderr[-600:]
    assert b"Number of output mappings (passed filters): %d\n" % lines in r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["out.bam"], "no header file is left behind"


def test_cli_bam_with_summary(tmp_path):
    import summary_fixtures as sf
    name = "s1_chip_sam"
    m = sf.meta(name)
    fa, reads, extra = sf.inputs(name)
    out, csv = str(tmp_path / "out.bam"), str(tmp_path / "summary.csv")
    r = subprocess.run([CLI] + m["chromap_flags"] + extra + ["--BAM", "-x", datasets.case_index(m["base_case"]), "-r", fa] + reads +
                       ["-o", out, "--summary", csv], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert open(csv, "rb").read() == sf.csv(name)
    if m["golden_output"]:
        _check_bam_file(open(out, "rb").read(), m["golden_output"])


@pytest.mark.skipif(shutil.which("samtools") is None, reason="samtools is not installed")
def test_samtools_reads_the_file(tmp_path):
    case = "s1_chip_sam"
    out = str(tmp_path / "out.bam")
    r = subprocess.run([CLI] + _cli_args(case) + ["--BAM", "-o", out], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert subprocess.run(["samtools", "quickcheck", out]).returncode == 0
    view = subprocess.run(["samtools", "view", "-h", "--no-PG", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert view.returncode == 0, view.stderr
    assert view.stdout == bm.normalise(_golden(case)[0])
