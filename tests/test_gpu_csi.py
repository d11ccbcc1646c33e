"""The CSI index built on the device (chromap_amd/csrc/cm_tabix.h, cm_bai.h, cm_tabix.hip), both flavours: for every record set
(tests/bai_records.py, tests/csi_cases.py) and every text (tests/tbi_texts.py, tests/csi_cases.py) the payload is the plain-Python
model's (tests/csi_model.py), byte for byte, the same from run to run, and region queries through it -- with the specification's
reader, min_off from the bins' loffsets -- return what a walk over the records or a scan of the text returns; what the .bai / .tbi
refuse for ends beyond 2^29 is indexed at depth 6; another base offset moves every virtual offset, the loffsets among them, and
leaves the pseudo-bin's loffset 0; what cannot be indexed is refused in the .bai's / .tbi's words, the limit named by the depth, and
the context goes on working.
More than 256 records (more than one block of the per-record kernels): records_767 / 768 / 769, one_position_1000,
bins_a_b_a_far and long_reference_515.  Records across a 0xff00 slice seam: block_seams, ends_on_a_seam and bins_a_b_a_far of
bai_records; lines across one: line_straddles_slice, line_begins_at_slice, exactly_two_slices of tbi_texts."""
import gzip
import random
import shutil
import subprocess

import pytest

import bai_model as bai
import bai_records as br
import bgzf_texts as bt
import csi_cases as cc
import csi_model as cm
import datasets
import tbi_texts as tt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from chromap_amd import ChromapGPU
    meta = datasets.case_meta("toy_atac")
    fa, _, _ = datasets.case_inputs("toy_atac")
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    g = ChromapGPU(datasets.case_index("toy_atac"), fa, preset=preset, **kw)
    yield g
    g.close()


def _moved(a, b, shift):
    """index b is index a with every virtual offset `shift` further; the pseudo-bin's loffset is 0 in both (parse_csi)"""
    assert len(a["refs"]) == len(b["refs"]) and a["aux"] == b["aux"]
    for ra, rb in zip(a["refs"], b["refs"]):
        assert rb["order"] == ra["order"] and rb["bins"] == {k: [(x + shift, y + shift) for x, y in ch] for k, ch in ra["bins"].items()}
        assert rb["loff"] == {k: v + shift for k, v in ra["loff"].items()}
        assert (rb["pseudo"] is None) == (ra["pseudo"] is None)
        if ra["pseudo"]:
            assert rb["pseudo"] == (ra["pseudo"][0] + shift, ra["pseudo"][1] + shift) + ra["pseudo"][2:]


def _bam(gpu, rs, depth, regions=None):
    """compress, index twice, index at another base; the payload must be the model's and answer the queries"""
    blocks = gpu.bgzf_compress(rs.data)
    head = rs.header_blocks()
    raw = head + blocks + bt.EOF_BLOCK
    payload = gpu.bgzf_csi(len(head), rs.n_ref, rs.starts, depth=depth)
    assert payload == cm.bam_model(raw, depth), "the device's index differs from the model's"
    assert gpu.bgzf_csi(len(head), rs.n_ref, rs.starts, depth=depth) == payload, "two runs, two results"
    _moved(cm.parse_csi(payload), cm.parse_csi(gpu.bgzf_csi(4711, rs.n_ref, rs.starts, depth=depth)), (4711 - len(head)) << 16)
    return cm.check_bam_queries(raw, payload, cc.regions(rs, depth) if regions is None else regions), payload


def _bed(gpu, text, depth, queries):
    comp = gpu.bgzf_compress(text)
    payload = gpu.bgzf_csi(0, depth=depth, kind="bed")
    assert payload == cm.bed_model(text, bt.blocks(comp), 0, depth), "the device's index differs from the model's"
    assert gpu.bgzf_csi(0, depth=depth, kind="bed") == payload, "two runs, two results"
    moved = gpu.bgzf_csi(4711, depth=depth, kind="bed")
    assert moved == cm.bed_model(text, bt.blocks(comp), 4711, depth)
    _moved(cm.parse_csi(payload), cm.parse_csi(moved), 4711 << 16)
    return cm.check_bed_queries(comp + bt.EOF_BLOCK, payload, text, queries) if text else 0, payload


# ---- 1. the sets and texts of the .bai's and .tbi's tests, at depth 5 and 6
@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("name", br.good())
def test_record_sets(gpu, name, depth):
    found, _ = _bam(gpu, br.sets()[name], depth)
    assert found or name == "empty"


@pytest.mark.parametrize("depth", [5, 6])
@pytest.mark.parametrize("name", sorted({**tt.small_texts(), **tt.edge_texts()}) + ["ladder", "big"])
def test_texts(gpu, name, depth):
    text = {**tt.small_texts(), **tt.edge_texts(), "ladder": tt.ladder_text()}[name] if name != "big" else tt.big_text()
    queries = tt.ladder_queries() if name == "ladder" else tt.random_queries(text, 25) if text else []
    found, payload = _bed(gpu, text, depth, queries)
    assert found or name == "empty"
    if name == "empty":
        assert len(payload) == 16 + 28 + 4 + 8


# ---- 2. what the .bai / .tbi refuse for ends beyond 2^29 is indexed at depth 6
def test_beyond_2_29_is_indexed_at_depth_6(gpu):
    from chromap_amd import ChromapError
    ranged = [n for n in br.refused() if br.sets()[n].refused[0] == bai.RANGE]
    assert ranged == ["refused_end_beyond"]
    for name in ranged:
        rs = br.sets()[name]
        gpu.bgzf_compress(rs.data)
        with pytest.raises(ChromapError) as e:
            gpu.bgzf_csi(0, rs.n_ref, rs.starts, depth=5)
        assert "record %d " % rs.refused[1] in str(e.value) and "2^29" in str(e.value), str(e.value)
        f = bai.File(rs.file(bai.bgzf_blocks_of(rs.data)))
        regions = [(rid, p, p + 1) for _, _, rid, pos, end, _ in bai.records(f) for p in (pos, end - 1, end)] + [(0, 0, 0xffffffff), (0, 1 << 29, (1 << 29) + 1)]
        found, _ = _bam(gpu, rs, 6, regions)
        assert found >= 3
    text, _, line, _ = tt.refused_texts()["end_beyond_2_29"]
    gpu.bgzf_compress(text)
    with pytest.raises(ChromapError) as e:
        gpu.bgzf_csi(0, depth=5, kind="bed")
    assert "line %d " % line in str(e.value) and "2^29" in str(e.value), str(e.value)
    found, _ = _bed(gpu, text, 6, [(b"chr2", 1 << 29, (1 << 29) + 1), (b"chr2", (1 << 29) - 1, 1 << 29), (b"chr2", 1 << 28, (1 << 28) + 1), (b"chr2", 0, 0xffffffff)]
                    + tt.random_queries(text, 25))
    assert found > 50


# ---- 3. other depths, bins beyond 16 bits, positions up to 2^32
@pytest.mark.parametrize("name", sorted(n for n, (rs, _) in cc.record_sets().items() if not rs.refused))
def test_csi_record_sets(gpu, name):
    rs, depth = cc.record_sets()[name]
    found, payload = _bam(gpu, rs, depth)
    assert found > 0
    idx = cm.parse_csi(payload)
    if name == "wide_bins":   # equal keys where the bin has 16 bits of the key: each bin under its own reference
        assert 65536 + cc.X in idx["refs"][0]["bins"] and cc.X not in idx["refs"][0]["bins"]
        assert cc.X in idx["refs"][1]["bins"] and 65536 + cc.X not in idx["refs"][1]["bins"]
    if name == "depth1":
        assert sorted(idx["refs"][0]["bins"]) == [0, 1, 2, 8] and idx["refs"][0]["pseudo"][2:] == (5, 0)


@pytest.mark.parametrize("name", sorted(n for n, (rs, _) in cc.record_sets().items() if rs.refused))
def test_csi_record_sets_refused(gpu, name):
    from chromap_amd import ChromapError
    rs, depth = cc.record_sets()[name]
    gpu.bgzf_compress(rs.data)
    with pytest.raises(ChromapError) as e:
        gpu.bgzf_csi(0, rs.n_ref, rs.starts, depth=depth)
    assert "record %d " % rs.refused[1] in str(e.value) and "2^%d" % (14 + 3 * depth) in str(e.value), str(e.value)
    with pytest.raises(ChromapError, match="no CSI index"):
        gpu.store_write_csi("/dev/null")
    ok, d = cc.record_sets()["depth1"]   # the context goes on working
    assert _bam(gpu, ok, d)[0] > 0


@pytest.mark.parametrize("name", sorted(cc.texts()))
def test_csi_texts(gpu, name):
    text, depth, queries = cc.texts()[name]
    found, payload = _bed(gpu, text, depth, queries + tt.random_queries(text, 25))
    assert found > 0
    if name == "wide_bins":
        idx = cm.parse_csi(payload)
        assert 65536 + cc.X in idx["refs"][0]["bins"] and cc.X in idx["refs"][1]["bins"] and cc.X not in idx["refs"][0]["bins"]


@pytest.mark.parametrize("name", sorted(cc.REFUSED_TEXTS))
def test_csi_texts_refused(gpu, name):
    from chromap_amd import ChromapError
    text, depth, line = cc.REFUSED_TEXTS[name]
    gpu.bgzf_compress(text)
    with pytest.raises(ChromapError) as e:
        gpu.bgzf_csi(0, depth=depth, kind="bed")
    assert "line %d " % line in str(e.value) and ("4294967295" if depth == 6 else "2^%d" % (14 + 3 * depth)) in str(e.value), str(e.value)
    t, d, q = cc.texts()["depth1"]
    assert _bed(gpu, t, d, q)[0] > 0


# ---- 4. the other refusals keep their words; arguments
@pytest.mark.parametrize("name", [n for n in br.refused() if br.sets()[n].refused[0] != bai.RANGE])
def test_refused_sets_keep_their_words(gpu, name):
    from chromap_amd import ChromapError
    rs = br.sets()[name]
    gpu.bgzf_compress(rs.data)
    cause, record = rs.refused
    with pytest.raises(ChromapError) as e:
        gpu.bgzf_csi(0, rs.n_ref, rs.starts, depth=6)
    with pytest.raises(ChromapError) as b:
        gpu.bgzf_bai(0, rs.n_ref, rs.starts)
    assert str(e.value) == str(b.value) and "record %d " % record in str(e.value) and bai.CAUSES[cause] in str(e.value)


@pytest.mark.parametrize("name", sorted(set(tt.refused_texts()) - {"end_beyond_2_29"}))
def test_refused_texts_keep_their_words(gpu, name):
    from chromap_amd import ChromapError
    text, _, line, words = tt.refused_texts()[name]
    gpu.bgzf_compress(text)
    with pytest.raises(ChromapError) as e:
        gpu.bgzf_csi(0, depth=6, kind="bed")
    with pytest.raises(ChromapError) as b:
        gpu.bgzf_tabix()
    assert str(e.value) == str(b.value) and words in str(e.value) and "line %d " % line in str(e.value)


def test_arguments(gpu, tmp_path):
    from chromap_amd import ChromapError
    rs = br.sets()["cigars"]
    gpu.bgzf_compress(rs.data)
    for depth in (0, 7, 100):
        with pytest.raises(ChromapError, match="depth must be 1 .. 6"):
            gpu.bgzf_csi(0, rs.n_ref, rs.starts, depth=depth)
        with pytest.raises(ChromapError, match="depth must be 1 .. 6"):
            gpu.bgzf_csi(0, depth=depth, kind="bed")
        with pytest.raises(ChromapError, match="no CSI index"):
            gpu.store_write_csi(str(tmp_path / "none.csi"))
    with pytest.raises(ValueError):
        gpu.bgzf_csi(kind="vcf")
    with pytest.raises(ChromapError, match="no record starts were kept"):
        gpu.bgzf_csi(0, rs.n_ref, depth=5)
    # the .csi file: a BGZF stream that ends with the end-of-file block; the .bai of the same records is not touched by it
    head = rs.header_blocks()
    bai_before = gpu.bgzf_bai(len(head), rs.n_ref, rs.starts)
    payload = gpu.bgzf_csi(len(head), rs.n_ref, rs.starts, depth=6)
    path = str(tmp_path / "x.csi")
    gpu.store_write_csi(path)
    packed = open(path, "rb").read()
    assert gzip.decompress(packed) == payload and packed.endswith(bt.EOF_BLOCK) and packed.count(bt.EOF_BLOCK) == 1
    bt.blocks(packed)
    assert gpu.bgzf_bai(len(head), rs.n_ref, rs.starts) == bai_before == bai.model(head + gpu.store_bgzf() + bt.EOF_BLOCK)


# ---- 5. the golden cases end to end: render, compress, index
def test_golden_bam_case(tmp_path):
    import test_gpu_bai as tgb
    import test_gpu_bam as tb
    g, bc_len = tb._fill_stores("s1_chip_sam")
    try:
        g.bam_keep_starts(True)
        n, _ = g.store_format_bam(barcode_length=bc_len)
        g.store_compress_text()
        raw, base = tgb._bam_file(g, tmp_path)
        for depth in (5, 6):
            payload = g.bgzf_csi(base, depth=depth)
            assert payload == cm.bam_model(raw, depth), depth
            idx = cm.parse_csi(payload)
            assert sum(r["pseudo"][2] + r["pseudo"][3] for r in idx["refs"] if r["pseudo"]) == n > 0
            assert cm.check_bam_queries(raw, payload, tgb._regions_of(raw, "csi")) > 10
        assert g.bgzf_bai(base) == bai.model(raw)
    finally:
        g.close()


def test_golden_bed_case():
    import test_gpu_tabix as tx
    import tbi_model as tm
    g, _ = tx._map_into_store("b1_atac_bc")
    try:
        text = g.store_text()
        assert text == datasets.case_golden_bed("b1_atac_bc")
        g.store_compress_text()
        comp = g.store_bgzf()
        for depth in (5, 6):
            payload = g.bgzf_csi(depth=depth, kind="bed")
            assert payload == cm.bed_model(text, bt.blocks(comp), 0, depth), depth
            assert cm.check_bed_queries(comp + bt.EOF_BLOCK, payload, text, tt.random_queries(text, 100)) > 100
        assert g.bgzf_tabix() == tm.model(text, bt.blocks(comp), 0)
    finally:
        g.close()


# ---- 6. htslib's readers, where they are installed
@pytest.mark.skipif(shutil.which("samtools") is None, reason="samtools is not installed")
def test_samtools_reads_through_the_index(gpu, tmp_path):
    rs, depth = cc.record_sets()["long_reference_515"]
    blocks = gpu.bgzf_compress(rs.data)
    head = bai.bgzf_blocks_of(bai.bam_header(rs.n_ref, length=0x7fffffff))
    raw = head + blocks + bt.EOF_BLOCK
    out = str(tmp_path / "out.bam")
    open(out, "wb").write(raw)
    gpu.bgzf_csi(len(head), rs.n_ref, rs.starts, depth=depth)
    gpu.store_write_csi(out + ".csi")
    f = bai.File(raw)
    recs = bai.records(f)
    rnd = random.Random(11)
    for at, size, rid, pos, end, flag in rnd.sample(recs, 10):
        beg, stop = max(0, pos - rnd.randrange(3000)), end + rnd.randrange(3000)
        view = subprocess.run(["samtools", "view", "-c", out, "ref%d:%d-%d" % (rid, beg + 1, stop)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert view.returncode == 0, view.stderr
        assert int(view.stdout) == len(bai.brute(f, rid, beg, stop)), (rid, beg, stop)
    stats = subprocess.run(["samtools", "idxstats", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert stats.returncode == 0, stats.stderr
    for ln in stats.stdout.splitlines():
        c = ln.split(b"\t")
        if c[0] != b"*":
            t = int(c[0][3:])
            assert (int(c[2]), int(c[3])) == (sum(1 for x in recs if x[2] == t and not x[5] & 4), sum(1 for x in recs if x[2] == t and x[5] & 4))


@pytest.mark.skipif(shutil.which("tabix") is None, reason="tabix is not installed")
def test_tabix_reads_through_the_index(gpu, tmp_path):
    text, depth, queries = cc.texts()["end_4294967000"]
    comp = gpu.bgzf_compress(text)
    out = str(tmp_path / "out.bed.gz")
    open(out, "wb").write(comp + bt.EOF_BLOCK)
    gpu.bgzf_csi(0, depth=depth, kind="bed")
    gpu.store_write_csi(out + ".csi")
    import tbi_model as tm
    for name, beg, end in queries:
        r = subprocess.run(["tabix", out, "%s:%d-%d" % (name.decode(), beg + 1, end)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr
        assert r.stdout == b"".join(tm.brute(text, name, beg, end)), (name, beg, end)
