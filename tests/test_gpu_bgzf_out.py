"""BGZF output compressed on the device (chromap_amd/csrc/cm_deflate.h, cm_bgzf_out.hip): the blocks inflate to the text, have the
structure of the format, equal the host emulation's byte for byte and do not change from run to run; the text store compressed in place
inflates to itself; and chromap-amd --output-bgzf writes files that gzip, and the tool's own reader, turn back into the golden text."""
import gzip
import os
import subprocess

import pytest

import bgzf_texts as bt
import datasets

pytestmark = pytest.mark.gpu
CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")


def _case_gpu(case):
    from chromap_amd import ChromapGPU
    meta = datasets.case_meta(case)
    fa, r1, r2 = datasets.case_inputs(case)
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    return ChromapGPU(datasets.case_index(case), fa, preset=preset, **kw), r1, r2


@pytest.fixture(scope="module")
def gpu():
    g, _, _ = _case_gpu("toy_atac")
    yield g
    g.close()


def _both(gpu, text):
    import hostemu_deflate_lib as hd
    comp = gpu.bgzf_compress(text)
    n_slices = (len(text) + bt.SLICE - 1) // bt.SLICE
    assert gpu.bgzf_info() == (n_slices, len(comp), len(text))
    bt.check_bgzf(comp, text)
    assert comp == hd.deflate(text, 0), "the device's blocks differ from the host emulation's"
    assert gpu.bgzf_compress(text) == comp, "two runs, two results"
    return comp


@pytest.mark.parametrize("name", sorted(bt.small_texts()))
def test_small_texts(gpu, name):
    text = bt.small_texts()[name]
    comp = _both(gpu, text)
    if name == "len0":
        assert comp == b"" and gpu.bgzf_info() == (0, 0, 0)


@pytest.mark.parametrize("key", sorted(bt.GOLDEN_TEXTS))
def test_golden_texts(gpu, key):
    """(several hundred slices for the SAM text: more slices than workgroups of a launch take in one turn)"""
    _both(gpu, bt.golden_text(key))


def test_more_slices_than_a_launch_holds_and_an_unaligned_tail(gpu):
    """2048 slices go into one launch: 2100 slices of highly repetitive text (fast to compress and to check) take two, the second
    with a short last slice"""
    line = b"chr7\t55019017\t55019365\tN\t60\n"
    text = (line * ((2100 * bt.SLICE) // len(line) + 1))[:2099 * bt.SLICE + 12345]
    comp = gpu.bgzf_compress(text)
    assert gpu.bgzf_info() == (2100, len(comp), len(text))
    assert len(bt.blocks(comp)) == 2100
    assert gzip.decompress(comp) == text
    assert gpu.bgzf_compress(text) == comp


def _compressed_store_is_the_text(g):
    text = g.store_text()
    assert len(text) > 1000
    n_blocks, n_out = g.store_compress_text()
    comp = g.store_bgzf()
    assert len(comp) == n_out and g.bgzf_info() == (n_blocks, n_out, len(text))
    bt.check_bgzf(comp, text)
    assert g.store_text() == text, "compressing must leave the text store alone"
    return text, comp


def test_store_format_then_compress(tmp_path):
    import oracle_lib as ol
    from chromap_amd import _capi, bgzf_write_eof, bgzf_write_host_text
    case = "s1_atac"
    g, r1, r2 = _case_gpu(case)
    try:
        b1, o1 = ol.read_fastx(r1)
        b2, o2 = ol.read_fastx(r2)
        g.map_pairs(b1, o1, b2, o2)
        g.store_append_resident()
        g.store_format(_capi.TEXT_BED_PE)
        text, comp = _compressed_store_is_the_text(g)
        assert text == datasets.case_golden_bed(case)
        # the file: host text in stored blocks, the store's blocks, the end-of-file block
        path = str(tmp_path / "o.bed.gz")
        bgzf_write_host_text(path, b"# a header line\n")
        g.store_write_bgzf(path, append=True)
        bgzf_write_eof(path)
        raw = open(path, "rb").read()
        assert raw.endswith(bt.EOF_BLOCK) and raw.count(bt.EOF_BLOCK) == 1
        assert raw[47:-28] == comp and gzip.decompress(raw) == b"# a header line\n" + text
    finally:
        g.close()


def test_store_format_pairs_resident_then_compress():
    from chromap_amd import Stats
    case = "h1_hic"
    g, r1, r2 = _case_gpu(case)
    try:
        g.fastq_keep_names(0, True)
        n = g.fastq_scan(0, open(r1, "rb").read(), True)
        assert g.fastq_scan(1, open(r2, "rb").read(), True) == n
        g.fastq_take(0, n)
        g.fastq_take(1, n)
        g.fastq_commit(n, first_read_id=0, paired=True)
        g.map_resident(Stats())
        g.store_clear()
        g.store_append_resident()
        g.store_format_pairs_resident()
        text, _ = _compressed_store_is_the_text(g)
        assert datasets.case_golden_bed(case).endswith(text)
    finally:
        g.close()


def test_store_format_sam_then_compress():
    from chromap_amd import Stats
    case = "s1_chip_sam"
    g, r1, r2 = _case_gpu(case)
    try:
        g.fastq_keep_reads(True)
        n = g.fastq_scan(0, open(r1, "rb").read(), True)
        assert g.fastq_scan(1, open(r2, "rb").read(), True) == n
        g.fastq_take(0, n)
        g.fastq_take(1, n)
        g.fastq_commit(n, first_read_id=0, paired=True)
        g.map_resident(Stats())
        g.sam_store_clear()
        g.sam_store_append_resident()
        g.store_format_sam()
        text, _ = _compressed_store_is_the_text(g)
        assert datasets.case_golden_bed(case).endswith(text)
    finally:
        g.close()


# ---- the command line: one golden case per kind of output
def _cli_args(case):
    fa, r1, r2 = datasets.case_inputs(case)
    m = datasets.single_end_mate(case)
    reads = ["-1", r1, "-2", r2] if not m else ["-1", r1 if m == 1 else r2]
    if datasets.has_barcodes(case):
        bc, wl = datasets.case_barcode_inputs(case)
        reads += ["-b", bc, "--barcode-whitelist", wl]
    return list(datasets.case_meta(case)["chromap_flags"]) + ["-x", datasets.case_index(case), "-r", fa] + reads


CLI_CASES = {"bed": ("s1_atac", []), "bed_bc_translate": ("b1_atac_bc", None), "tagalign": ("s2_tagalign_q0", []), "pairs": ("h1_hic", []),
             "sam": ("s1_chip_sam", []), "bed_force_exchange": ("s1_atac", ["--force-exchange"])}


@pytest.mark.parametrize("kind", sorted(CLI_CASES))
def test_cli_output_bgzf(kind, tmp_path):
    case, extra = CLI_CASES[kind]
    want = datasets.case_golden_bed(case)
    if extra is None:  # column 4 through a translation table: the golden text translated by the model of the table
        import test_gpu_barcode_translate as tr
        _, wlf = datasets.case_barcode_inputs(case)
        table = tr.whitelist_table(wlf, str(tmp_path / "tr.tsv"), tr.CELL_NAME)
        want = tr.translate_bed(want, open(table, "rb").read(), len(want.split(b"\t")[3]))
        extra = ["--barcode-translate", table]
    out = str(tmp_path / "out.gz")
    r = subprocess.run([CLI] + _cli_args(case) + extra + ["--output-bgzf", "-o", out], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    raw = open(out, "rb").read()
    assert gzip.decompress(raw) == want
    if kind == "sam":
        assert want.startswith(b"@SQ")
    if kind == "pairs":
        assert want.startswith(b"## pairs format")
    assert raw.endswith(bt.EOF_BLOCK) and raw.count(bt.EOF_BLOCK) == 1
    for at, size in bt.blocks(raw[:-28]):
        assert size > 28, "an empty block in the middle of the file"
    assert b"bytes of BGZF on the device" in r.stderr
    import re
    m = re.search(rb"Compressed (\d+) bytes of text into (\d+) bytes of BGZF", r.stderr)
    assert (int(m.group(1)), int(m.group(2))) == (len(want), len(raw))
    back = subprocess.run([CLI, "--inflate-only", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert back.returncode == 0 and back.stdout == want and b"bgzf" in back.stderr
