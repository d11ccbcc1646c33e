"""The tabix index built on the device (chromap_amd/csrc/cm_tabix.h, cm_tabix.hip): for every text the payload is the sequential model's
(tests/tbi_model.py), byte for byte, the same from run to run, and region queries through it -- with a reader written from the
specification -- return what a scan of the text returns; texts that cannot be indexed are refused with a message that names the
cause and the line, and the context goes on working; chromap-amd --output-bgzf --output-tbi writes a .tbi that is the model of its
own output file."""
import gzip
import os
import re
import subprocess

import pytest

import bgzf_texts as bt
import datasets
import tbi_model as tm
import tbi_texts as tt

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


def _index(gpu, text, base=0):
    """compress, index twice; the payload must be the model's"""
    comp = gpu.bgzf_compress(text)
    sizes = bt.blocks(comp)
    payload = gpu.bgzf_tabix(base)
    assert payload == tm.model(text, sizes, base), "the device's index differs from the model's"
    assert gpu.bgzf_tabix(base) == payload, "two runs, two results"
    return comp, payload


@pytest.mark.parametrize("name", sorted(tt.small_texts()) + sorted(tt.edge_texts()))
def test_small_and_edge_texts(gpu, name):
    text = {**tt.small_texts(), **tt.edge_texts()}[name]
    comp, payload = _index(gpu, text)
    if name == "empty":
        assert comp == b"" and len(payload) == 44
    else:
        tt.check_queries(comp + bt.EOF_BLOCK, payload, text, tt.random_queries(text, 25))
    # the same text at another place in the file: every virtual offset moves with it
    assert gpu.bgzf_tabix(4711) == tm.model(text, bt.blocks(comp), 4711)


def test_bin_ladder(gpu):
    text = tt.ladder_text()
    comp, payload = _index(gpu, text)
    tt.check_queries(comp + bt.EOF_BLOCK, payload, text, tt.ladder_queries())


def test_more_slices_than_a_compressor_launch_holds(gpu):
    """2 048 slices go into one launch of the compressor: the block offsets behind them come from the second launch"""
    text = tt.big_text()
    comp, payload = _index(gpu, text)
    assert len(bt.blocks(comp)) > 2049
    edge = 2048 * bt.SLICE
    at = text.rindex(b"\n", 0, edge) + 1    # the line across (or at) the 2 048-slice boundary, and its neighbours
    cols = text[at:at + 64].split(b"\t")
    name, beg = cols[0], int(cols[1])
    queries = [(name, beg - 997 * k, beg - 997 * k + 1) for k in (-3, -2, -1, 0, 1, 2, 3)] + [(name, beg - 5000, beg + 5000), (b"chr1", 0, 1)]
    tt.check_queries(comp + bt.EOF_BLOCK, payload, text, queries)


def test_non_zero_base_in_a_file(gpu, tmp_path):
    """a header block written by the host, the store's blocks, the end-of-file block: the index points into the file"""
    from chromap_amd import bgzf_write_eof, bgzf_write_host_text
    text = tt.edge_texts()["name_runs_cross_slices"]
    header = b"# a comment line the index skips\n"
    comp = gpu.bgzf_compress(text)
    path = str(tmp_path / "o.bed.gz")
    bgzf_write_host_text(path, header)
    base = os.path.getsize(path)
    assert base == len(header) + 31
    gpu.store_write_bgzf(path, append=True)
    bgzf_write_eof(path)
    payload = gpu.bgzf_tabix(base)
    assert payload == tm.model(text, bt.blocks(comp), base)
    raw = open(path, "rb").read()
    assert gzip.decompress(raw) == header + text
    tt.check_queries(raw, payload, text, tt.random_queries(text, 40))
    tbi = path + ".tbi"
    gpu.store_write_tbi(tbi)
    packed = open(tbi, "rb").read()
    assert gzip.decompress(packed) == payload and packed.endswith(bt.EOF_BLOCK) and packed.count(bt.EOF_BLOCK) == 1
    bt.blocks(packed)


def _map_into_store(case):
    """the case's reads mapped and rendered as BED in the text store"""
    import oracle_lib as ol
    from chromap_amd import Stats, _capi
    g, r1, r2 = _case_gpu(case)
    if datasets.has_barcodes(case):
        bcf, wlf = datasets.case_barcode_inputs(case)
        _, _, bco = ol.read_fastq_qual(bcf)
        g.set_whitelist_file(wlf, int(bco[1] - bco[0]))
        bc, _, bco = ol.read_fastq_qual(bcf)
        g.compute_barcode_abundance(bc, bco)
        ns = [g.fastq_scan(s, open(f, "rb").read(), True) for s, f in ((0, r1), (1, r2), (2, bcf))]
        for s in range(3):
            g.fastq_take(s, ns[0])
        g.fastq_commit(ns[0], paired=True, barcoded=True)
        g.map_resident(Stats())
        g.store_clear()
        g.store_append_resident()
        render = lambda: g.store_format(_capi.TEXT_BED_PE_BC, barcode_length=g.barcode_length)
    else:
        b1, o1 = ol.read_fastx(r1)
        b2, o2 = ol.read_fastx(r2)
        g.map_pairs(b1, o1, b2, o2)
        g.store_append_resident()
        render = lambda: g.store_format(_capi.TEXT_BED_PE)
    render()
    return g, render


@pytest.mark.parametrize("case", ["s1_atac", "b1_atac_bc"])
def test_golden_store_format_then_compress_then_index(case):
    from chromap_amd import ChromapError
    g, render = _map_into_store(case)
    try:
        text = g.store_text()
        assert text == datasets.case_golden_bed(case)
        g.store_compress_text()
        comp = g.store_bgzf()
        payload = g.bgzf_tabix()
        assert payload == tm.model(text, bt.blocks(comp), 0)
        assert g.bgzf_tabix() == payload
        tt.check_queries(comp + bt.EOF_BLOCK, payload, text, tt.random_queries(text, 100))
        if case == "b1_atac_bc":
            assert len(payload) == 4920
        # a text store rendered anew is no longer what the blocks hold
        render()
        assert g.store_text() == text
        with pytest.raises(ChromapError, match="rendered anew"):
            g.bgzf_tabix()
        g.store_compress_text()
        assert g.bgzf_tabix() == payload
    finally:
        g.close()


def test_index_without_a_compressed_store():
    from chromap_amd import ChromapError
    g, _, _ = _case_gpu("toy_atac")
    try:
        with pytest.raises(ChromapError, match="no compressed store"):
            g.bgzf_tabix()
        with pytest.raises(ChromapError, match="no tabix index"):
            g.store_write_tbi("/dev/null")
        _index(g, tt.small_texts()["one_line"])
    finally:
        g.close()


@pytest.mark.parametrize("name", sorted(tt.refused_texts()))
def test_refusals_name_the_cause_and_leave_the_context_usable(gpu, name):
    from chromap_amd import ChromapError
    text, _, line, words = tt.refused_texts()[name]
    comp = gpu.bgzf_compress(text)
    assert gzip.decompress(comp) == text
    with pytest.raises(ChromapError) as e:
        gpu.bgzf_tabix()
    assert words in str(e.value) and "line %d " % line in str(e.value), str(e.value)
    with pytest.raises(ChromapError, match="no tabix index"):
        gpu.store_write_tbi("/dev/null")
    good = tt.small_texts()["one_bin"]
    _index(gpu, good)


def test_paired_tagalign_text_is_refused(gpu):
    from chromap_amd import ChromapError
    text = datasets.case_golden_bed("s2_tagalign_q0")
    gpu.bgzf_compress(text)
    with pytest.raises(ChromapError, match="not sorted by start") as e:
        gpu.bgzf_tabix()
    with pytest.raises(tm.NotIndexable) as m:
        tm.model(text, [28] * ((len(text) + bt.SLICE - 1) // bt.SLICE), 0)
    assert "line %d " % m.value.line in str(e.value)


# ---- the command line
def _cli_args(case):
    fa, r1, r2 = datasets.case_inputs(case)
    m = datasets.single_end_mate(case)
    reads = ["-1", r1, "-2", r2] if not m else ["-1", r1 if m == 1 else r2]
    if datasets.has_barcodes(case):
        bc, wl = datasets.case_barcode_inputs(case)
        reads += ["-b", bc, "--barcode-whitelist", wl]
    return list(datasets.case_meta(case)["chromap_flags"]) + ["-x", datasets.case_index(case), "-r", fa] + reads


CLI_CASES = {"bed": ("s1_atac", []), "bed_bc": ("b1_atac_bc", []), "bed_bc_translate": ("b1_atac_bc", None), "tagalign_se": ("s4_se_tagalign_q0", []),
             "tagalign_se_bc": ("b1_se_bc_tagalign_q0", [])}


@pytest.mark.parametrize("kind", sorted(CLI_CASES))
def test_cli_output_tbi(kind, tmp_path):
    case, extra = CLI_CASES[kind]
    want = datasets.case_golden_bed(case)
    if extra is None:
        import test_gpu_barcode_translate as tr
        _, wlf = datasets.case_barcode_inputs(case)
        table = tr.whitelist_table(wlf, str(tmp_path / "tr.tsv"), tr.CELL_NAME)
        want = tr.translate_bed(want, open(table, "rb").read(), len(want.split(b"\t")[3]))
        extra = ["--barcode-translate", table]
    out = str(tmp_path / "out.bed.gz")
    r = subprocess.run([CLI] + _cli_args(case) + extra + ["--output-bgzf", "--output-tbi", "-o", out], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    raw = open(out, "rb").read()
    assert gzip.decompress(raw) == want
    assert raw.endswith(bt.EOF_BLOCK) and raw.count(bt.EOF_BLOCK) == 1
    packed = open(out + ".tbi", "rb").read()
    assert packed.endswith(bt.EOF_BLOCK) and packed.count(bt.EOF_BLOCK) == 1
    bt.blocks(packed)
    payload = gzip.decompress(packed)
    assert payload == tm.model(want, bt.blocks(raw[:-28]), 0)
    tt.check_queries(raw, payload, want, tt.random_queries(want, 60))
    m = re.search(rb"wrote (\S+) \((\d+) bytes before compression\)", r.stderr)
    assert m and m.group(1).decode() == out + ".tbi" and int(m.group(2)) == len(payload)
    assert sorted(os.listdir(tmp_path)) == sorted(["out.bed.gz", "out.bed.gz.tbi"] + (["tr.tsv"] if kind == "bed_bc_translate" else []))
