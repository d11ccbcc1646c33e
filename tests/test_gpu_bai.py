"""The BAM index built on the device (chromap_amd/csrc/cm_bai.h, cm_tabix.hip): for every synthetic record set (tests/bai_records.py)
and for the BAM records of the golden SAM cases the payload is the plain-Python model's (tests/bai_model.py) of the whole file, byte
for byte, the same from run to run, and region queries through it return what a walk over the records returns; records that cannot
be indexed are refused with a message that names the cause and the record, and the context goes on working; the record starts
cmgpu_store_format_bam keeps belong to one rendering; chromap-amd --BAM --output-bai writes a .bai that is the model of its own
output file, beside a BAM file that is the one it writes without the flag."""
import os
import random
import shutil
import subprocess

import pytest

import bai_model as bai
import bai_records as br
import bgzf_texts as bt
import datasets

pytestmark = pytest.mark.gpu
CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")
CASES = ["s1_chip_sam", "s1_se_sam", "b1_bc_sam", "h1_hic_sam", "x2_gaps_sam_q0"]


@pytest.fixture(scope="module")
def gpu():
    from chromap_amd import ChromapGPU
    meta = datasets.case_meta("toy_atac")
    fa, _, _ = datasets.case_inputs("toy_atac")
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    g = ChromapGPU(datasets.case_index("toy_atac"), fa, preset=preset, **kw)
    yield g
    g.close()


@pytest.fixture(scope="module")
def stores():
    import test_gpu_bam as tb
    made = {}

    def get(case):
        if case not in made:
            made[case] = tb._fill_stores(case)
        return made[case]
    yield get
    for g, _ in made.values():
        g.close()


def _check_queries(raw, payload, regions):
    f = bai.File(raw)
    index, n_no_coor = bai.parse_bai(payload)
    assert n_no_coor == 0 and len(index) == f.n_ref
    found = 0
    for tid, beg, end in regions:
        want = bai.brute(f, tid, beg, end)
        assert bai.query(f, index, tid, beg, end) == want, (tid, beg, end)
        found += len(want)
    return found


# ---- 1. the synthetic sets: records the test compresses itself, their starts handed over
@pytest.mark.parametrize("name", br.good())
def test_synthetic_sets(gpu, name):
    rs = br.sets()[name]
    blocks = gpu.bgzf_compress(rs.data)
    head = rs.header_blocks()
    raw = head + blocks + bt.EOF_BLOCK
    payload = gpu.bgzf_bai(len(head), rs.n_ref, rs.starts)
    assert payload == bai.model(raw), "the device's index differs from the model's"
    assert gpu.bgzf_bai(len(head), rs.n_ref, rs.starts) == payload, "two runs, two results"
    # the same records behind another header: every virtual offset moves with it
    moved = gpu.bgzf_bai(4711, rs.n_ref, rs.starts)
    a, b = bai.parse_bai(payload)[0], bai.parse_bai(moved)[0]
    shift = (4711 - len(head)) << 16
    for ra, rb in zip(a, b):
        assert rb["lin"] == [v + shift for v in ra["lin"]] and rb["order"] == ra["order"]
        assert rb["bins"] == {k: [(x + shift, y + shift) for x, y in ch] for k, ch in ra["bins"].items()}
        assert (rb["pseudo"] is None) == (ra["pseudo"] is None)
    found = _check_queries(raw, payload, br.regions(rs))
    assert found or name == "empty"


@pytest.mark.parametrize("name", br.refused())
def test_refused_sets(gpu, name):
    from chromap_amd import ChromapError
    rs = br.sets()[name]
    gpu.bgzf_compress(rs.data)
    cause, record = rs.refused
    with pytest.raises(ChromapError) as e:
        gpu.bgzf_bai(0, rs.n_ref, rs.starts)
    assert "record %d " % record in str(e.value) and bai.CAUSES[cause] in str(e.value), str(e.value)
    if cause == bai.RANGE:
        assert "samtools index -c" in str(e.value)
    # the context goes on working
    ok = br.sets()["cigars"]
    blocks = gpu.bgzf_compress(ok.data)
    head = ok.header_blocks()
    assert gpu.bgzf_bai(len(head), ok.n_ref, ok.starts) == bai.model(head + blocks + bt.EOF_BLOCK)


# ---- 2. the golden cases: the records cmgpu_store_format_bam writes, the starts it keeps
def _bam_file(g, tmp_path):
    """(file bytes, base) of the compressed store behind the header's blocks"""
    path = str(tmp_path / "header.bin")
    g.write_bam_header(path)
    head = bai.bgzf_blocks_of(open(path, "rb").read())
    return head + g.store_bgzf() + bt.EOF_BLOCK, len(head)


def _regions_of(raw, seed):
    f = bai.File(raw)
    recs = bai.records(f)
    rnd = random.Random(seed)
    out = []
    for at, size, rid, pos, end, flag in rnd.sample(recs, min(10, len(recs))):
        out += [(rid, pos, pos + 1), (rid, end - 1, end), (rid, end, end + 1), (rid, max(0, pos - 1), pos), (rid, max(0, pos - 20000), end + 20000)]
    out += [(rnd.randrange(f.n_ref), b, b + w) for b, w in ((rnd.randrange(1 << 22), rnd.choice((1, 500, 1 << 14, 1 << 20))) for _ in range(15))]
    return out


@pytest.mark.parametrize("case", CASES)
def test_golden_cases(case, stores, tmp_path):
    from chromap_amd import _capi
    g, bc_len = stores(case)
    g.bam_keep_starts(True)
    sizes, want = set(), {}
    try:
        for dedup, thr in ((0, None), (1, 30)):
            p = _capi.Params.from_buffer_copy(g.params)
            if dedup:   # unselected records lie between the selected ones: the kept starts are a compaction
                p.remove_pcr_duplicates, p.mapq_threshold = 1, thr
            for group in (8, 16, 64):
                g.set_option("sam_format_group", group)
                n, nbytes = g.store_format_bam(params=p, barcode_length=bc_len)
                g.store_compress_text()
                raw, base = _bam_file(g, tmp_path)
                payload = g.bgzf_bai(base)
                if raw not in want:   # (the group width does not change the file: one model per selection)
                    want[raw] = bai.model(raw)
                assert payload == want[raw], (dedup, group)
                counted = sum(r["pseudo"][2] + r["pseudo"][3] for r in bai.parse_bai(payload)[0] if r["pseudo"])
                assert counted == n > 0, (dedup, group)
                sizes.add(n)
                if group == 8 and not dedup:
                    assert _check_queries(raw, payload, _regions_of(raw, case)) > 10
    finally:
        g.set_option("sam_format_group", 8)
        g.bam_keep_starts(False)
    assert min(sizes) < g.sam_store_info()[0], "the selection drops records here: the kept starts are fewer than the store's records"


# ---- 3. kept starts belong to one rendering
def test_stale_and_missing_starts(stores, tmp_path):
    from chromap_amd import ChromapError, _capi
    case = "s1_chip_sam"
    g, bc_len = stores(case)
    g.bam_keep_starts(False)
    g.store_format_bam(barcode_length=bc_len)
    g.store_compress_text()
    with pytest.raises(ChromapError, match="no record starts were kept"):
        g.bgzf_bai()
    g.bam_keep_starts(True)
    try:
        with pytest.raises(ChromapError, match="no record starts were kept"):
            g.bgzf_bai()   # (turning it on does not bring back what the rendering before did not keep)
        n_all, _ = g.store_format_bam(barcode_length=bc_len)
        with pytest.raises(ChromapError, match="rendered anew"):
            g.bgzf_bai()   # (not compressed yet)
        g.store_compress_text()
        raw, base = _bam_file(g, tmp_path)
        first = g.bgzf_bai(base)
        assert first == bai.model(raw)
        # SAM text in the same store: neither the blocks nor the starts are its own
        g.store_format_sam(barcode_length=bc_len)
        with pytest.raises(ChromapError, match="rendered anew"):
            g.bgzf_bai(base)
        g.store_compress_text()
        with pytest.raises(ChromapError, match="does not hold BAM records"):
            g.bgzf_bai(base)
        # a second rendering: the index follows it
        p = _capi.Params.from_buffer_copy(g.params)
        p.remove_pcr_duplicates, p.mapq_threshold = 0, 0   # (the case's own flags remove duplicates and filter at 30)
        n_more, _ = g.store_format_bam(params=p, barcode_length=bc_len)
        assert n_more > n_all
        g.store_compress_text()
        raw2, base2 = _bam_file(g, tmp_path)
        second = g.bgzf_bai(base2)
        assert second == bai.model(raw2) and second != first
        # records of the caller's own in the compressed store: the kept starts are not theirs
        rs = br.sets()["cigars"]
        g.bgzf_compress(rs.data)
        with pytest.raises(ChromapError, match="no record starts were kept"):
            g.bgzf_bai(0, rs.n_ref)
        head = rs.header_blocks()
        own = g.bgzf_bai(len(head), rs.n_ref, rs.starts)
        assert own == bai.model(rs.file(g.store_bgzf()))
        path = str(tmp_path / "x.bai")
        g.store_write_bai(path)
        assert open(path, "rb").read() == own
    finally:
        g.bam_keep_starts(False)


# ---- 4. the command line
@pytest.mark.parametrize("case", ["s1_chip_sam", "b1_bc_sam"])
def test_cli_output_bai(case, tmp_path):
    import test_gpu_bam as tb
    out = str(tmp_path / "out.bam")
    r = subprocess.run([CLI] + tb._cli_args(case) + ["--BAM", "--output-bai", "-o", out], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert sorted(os.listdir(str(tmp_path))) == ["out.bam", "out.bam.bai"]
    raw = open(out, "rb").read()
    payload = open(out + ".bai", "rb").read()
    assert payload == bai.model(raw)
    assert b"Built the BAM index on the device and wrote %s.bai (%d bytes) in " % (out.encode(), len(payload)) in r.stderr, r.stderr[-600:]
    assert _check_queries(raw, payload, _regions_of(raw, case)) > 10
    plain = str(tmp_path / "plain.bam")
    r = subprocess.run([CLI] + tb._cli_args(case) + ["--BAM", "-o", plain], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert open(plain, "rb").read() == raw, "the flag changes the BAM file"
    assert sorted(os.listdir(str(tmp_path))) == ["out.bam", "out.bam.bai", "plain.bam"]


@pytest.mark.skipif(shutil.which("samtools") is None, reason="samtools is not installed")
def test_samtools_reads_through_the_index(tmp_path):
    import test_gpu_bam as tb
    case = "s1_chip_sam"
    out = str(tmp_path / "out.bam")
    r = subprocess.run([CLI] + tb._cli_args(case) + ["--BAM", "--output-bai", "-o", out], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    raw = open(out, "rb").read()
    f = bai.File(raw)
    recs = bai.records(f)
    names = [ln.split(b"\t")[1][3:] for ln in f.data[8:f.first_record].split(b"\n") if ln.startswith(b"@SQ")]
    rnd = random.Random(11)
    for at, size, rid, pos, end, flag in rnd.sample(recs, 10):
        beg, stop = max(0, pos - rnd.randrange(3000)), end + rnd.randrange(3000)
        view = subprocess.run(["samtools", "view", "-c", out, "%s:%d-%d" % (names[rid].decode(), beg + 1, stop)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert view.returncode == 0, view.stderr
        assert int(view.stdout) == len(bai.brute(f, rid, beg, stop)), (rid, beg, stop)
    stats = subprocess.run(["samtools", "idxstats", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert stats.returncode == 0, stats.stderr
    for ln in stats.stdout.splitlines():
        c = ln.split(b"\t")
        if c[0] != b"*":
            t = names.index(c[0])
            assert (int(c[2]), int(c[3])) == (sum(1 for x in recs if x[2] == t and not x[5] & 4), sum(1 for x in recs if x[2] == t and x[5] & 4))
