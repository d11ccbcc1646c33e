"""Layout CMGPU_FASTX_FREE of the device FASTQ ingest (cm_ingest.hip, cm_fastx.h): wrapped FASTQ, FASTA reads and stray blank lines give
the batches a byte-level model of kseq_read gives (fastx_layouts.Kseq), for any chunking of the text and for BGZF inflated on the device;
plain four-line text never leaves the four-line path; through the CLI the re-laid-out inputs of golden cases reproduce the committed
outputs of the reference."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import datasets as ds
import fastx_layouts as fx

pytestmark = pytest.mark.gpu
CLI = os.path.join(ds.ROOT, "chromap_amd", "chromap-amd")
REF = os.path.join(ds.ROOT, "oracle", "_ref", "chromap")
GEN = os.path.join(ds.ROOT, "tools", "gen_synth.py")


@pytest.fixture(scope="module")
def gpu():
    from chromap_amd import ChromapGPU
    fa, _, _ = ds.case_inputs("toy_chip")
    g = ChromapGPU(ds.case_index("toy_chip"), fa, preset="chip")
    yield g
    g.close()


def _split(b, off):
    raw = b.tobytes()
    return [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def _ingest_stream(g, text, chunk, stream=0, limit=None, first=0):
    """feeds `text` in chunks of `chunk` bytes the way the CLI does; returns the sequences taken, batch by batch"""
    seqs = []
    pos, carry = 0, b""
    while True:
        piece = text[pos:pos + chunk]
        pos += len(piece)
        final = pos >= len(text)
        buf = carry + piece
        n = g.fastq_scan(stream, buf, final)
        k = min(n, limit) if limit else n
        used = g.fastq_take(stream, k)
        if k:
            g.fastq_commit(k, first_read_id=first + len(seqs), paired=False)
            b1, o1, _, _ = g.download_batch(k)
            seqs += _split(b1, o1)
        carry = buf[used:]
        if final and k == n:
            assert carry == b"", "a final chunk is consumed whole"
            break
    return seqs


def _bgzf_blocks(text, level=1, block=0xff00):
    sys.path.insert(0, os.path.join(ds.ROOT, "tools"))
    import bgzf
    return [bgzf._block(text[i:i + block], level) for i in range(0, len(text), block)] + [bgzf._block(b"", level)]


def _ingest_bgzf(g, blocks, per_call, stream=0):
    """feeds the blocks `per_call` at a time; the device keeps what a take leaves"""
    seqs = []
    at = 0
    while True:
        piece = b"".join(blocks[at:at + per_call])
        at += per_call
        final = at >= len(blocks)
        n = g.fastq_scan(stream, piece, final, bgzf=True)
        g.fastq_take(stream, n)
        if n:
            g.fastq_commit(n, paired=False)
            b1, o1, _, _ = g.download_batch(n)
            seqs += _split(b1, o1)
        if final:
            break
    return seqs


def _fresh(g):
    """leaves device mode (a plain-text scan drops retained text) so that the layout may change"""
    g.fastq_scan(0, b"@a\nAC\n+\nII\n", True)
    g.fastq_take(0, 1)


def test_hand_made_layouts_for_every_chunking(gpu):
    from chromap_amd import FASTX_FREE, FASTX_STRICT4
    g = gpu
    g.fastq_set_layout(0, FASTX_FREE)
    for label, text in fx.hand_made():
        _, want, _, trunc = fx.expected(text)
        assert not trunc
        for chunk in (4096, 100003, max(1, len(text))):
            assert _ingest_stream(g, text, chunk) == want, (label, chunk)
        blocks = _bgzf_blocks(text, 1, 5000)
        for per_call in (1, 7, len(blocks)):
            assert _ingest_bgzf(g, blocks, per_call) == want, (label, "bgzf", per_call)
        _fresh(g)
    assert _ingest_stream(g, fx.hand_made()[2][1], 3000, limit=7) == fx.expected(fx.hand_made()[2][1])[1]
    g.fastq_set_layout(0, FASTX_STRICT4)


def test_two_hundred_generated_texts(gpu):
    from chromap_amd import FASTX_FREE, FASTX_STRICT4
    g = gpu
    g.fastq_set_layout(0, FASTX_FREE)
    general = 0
    for seed in range(200):
        text = fx.accepted_text(seed)
        _, want, _, trunc = fx.expected(text)
        assert not trunc
        for chunk in (4096, 100003, max(1, len(text))):
            assert _ingest_stream(g, text, chunk) == want, (seed, chunk, text)
        general += g.fastq_scan_info(0)[0]
        blocks = _bgzf_blocks(text, 6, 700)
        for per_call in (1, 7, len(blocks)):
            assert _ingest_bgzf(g, blocks, per_call) == want, (seed, "bgzf", per_call, text)
        _fresh(g)
    assert general > 100
    g.fastq_set_layout(0, FASTX_STRICT4)


def test_names_and_whole_reads_of_free_layouts(gpu):
    from chromap_amd import FASTX_FREE, FASTX_STRICT4, ChromapError
    g = gpu
    g.fastq_set_layout(0, FASTX_FREE)
    cases = fx.hand_made()
    g.fastq_keep_names(0, True)
    for label, text in cases:
        wn, ws, _, _ = fx.expected(text)
        g.names_clear()
        assert _ingest_stream(g, text, 4096) == ws, label
        assert g.download_names() == wn, label
    g.fastq_keep_names(0, False)
    g.names_clear()
    g.fastq_keep_reads(True)
    n_fastq = 0
    for label, text in cases:
        wn, ws, wq, _ = fx.expected(text)
        g.reads_clear()
        if any(q is None for q in wq):  # FASTA: whole reads need qualities, as the reference's SAM writer does
            with pytest.raises(ChromapError, match="reference cannot write SAM for FASTA"):
                _ingest_stream(g, text, 1 << 30)
            continue
        n_fastq += 1
        for chunk in (4096, 1 << 30):
            g.reads_clear()
            assert _ingest_stream(g, text, chunk) == ws, label
            names, bases, quals, off = g.download_reads(0)
            assert names == wn and _split(bases, off) == ws and _split(quals, off) == wq, (label, chunk)
    assert n_fastq >= 15
    # --read-format on wrapped records: ranges and the '-' strand apply to the concatenation
    recs = fx.toy_records(300, 21, 40, 90)
    comp = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")
    starts, ends = np.array([3, 30], np.int32), np.array([11, -1], np.int32)
    assert g.L.cmgpu_fastq_set_format(g.ctx, 0, 2, starts.ctypes.data, ends.ctypes.data, b"-") == 0
    g.reads_clear()
    got = _ingest_stream(g, fx.render(recs, width=7, blanks=(0, 2)), 4096)
    _, bases, quals, off = g.download_reads(0)
    want_s = [bytes(c if c in b"ACGTacgt" else ord("N") for c in (s[3:12] + s[30:])[::-1]).upper().translate(comp) for _, s, _ in recs]
    assert got == want_s and _split(bases, off) == want_s
    assert _split(quals, off) == [(q[3:12] + q[30:])[::-1] for _, _, q in recs]
    assert g.L.cmgpu_fastq_set_format(g.ctx, 0, 0, None, None, b"+") == 0
    g.fastq_keep_reads(False)
    g.reads_clear()
    g.fastq_set_layout(0, FASTX_STRICT4)


def test_four_line_text_stays_on_the_four_line_path(gpu):
    from chromap_amd import FASTX_FREE, FASTX_STRICT4, ChromapError
    g = gpu
    _, r1, _ = ds.case_inputs("s2_atac_q0")
    text = open(r1, "rb").read()
    strict = _ingest_stream(g, text, 1 << 30)
    assert g.fastq_scan_info(0)[0] == 0
    g.fastq_set_layout(0, FASTX_FREE)
    n = g.fastq_scan(0, text, True)
    general, n_lines = g.fastq_scan_info(0)
    assert general == 0 and n_lines == text.count(b"\n") and n == len(strict)
    g.fastq_take(0, n)
    for chunk in (1 << 30, 100003):
        assert _ingest_stream(g, text, chunk) == strict
        assert g.fastq_scan_info(0)[0] == 0
    # the same reads wrapped: the general path, the same batch
    recs = [(b"r%d" % i, s, b"I" * len(s)) for i, s in enumerate(strict)]
    assert _ingest_stream(g, fx.render(recs, width=33), 1 << 22) == strict
    assert g.fastq_scan_info(0)[0] == 1
    # a quality of another length is kseq's -2 for every stream in this layout
    with pytest.raises(ChromapError, match="truncated quality"):
        g.fastq_scan(0, b"@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGTACGT\n+\nIIII\n@c\nACGT\n+\nIIII\n", True)
    with pytest.raises(ChromapError, match="where a record is looked for"):
        g.fastq_scan(0, b"@a\nACGT\n+\nIIII\njunk\n@b\nAC\n+\nII\n", True)
    # unknown layouts, and a change while inflated text is retained
    with pytest.raises(ChromapError):
        g.fastq_set_layout(0, 7)
    blocks = _bgzf_blocks(b"@a\nACGT\n+\nIIII\n@b\nAC", 6)
    assert g.fastq_scan(0, b"".join(blocks), False, bgzf=True) == 1
    g.fastq_take(0, 1)
    with pytest.raises(ChromapError, match="kept on the device"):
        g.fastq_set_layout(0, FASTX_STRICT4)
    g.fastq_set_layout(0, FASTX_FREE)  # (no change: fine)
    _fresh(g)
    g.fastq_set_layout(0, FASTX_STRICT4)
    # the default layout refuses wrapped text with the four-line message
    with pytest.raises(ChromapError, match="4-line FASTQ"):
        g.fastq_scan(0, b"@a\nACGT\nACGT\n+\nIIIIIIII\n@b\nAC\n+\nII\n", True)


# ---- end to end through the CLI ----
def _records(path):
    lines = open(path, "rb").read().split(b"\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def _relayout(path, out, how):
    recs = _records(path)
    if how == "wrapped":
        t = fx.render(recs, width=33, plus_name=True, blanks=(0, 1, 0, 3), lead=1, trail=2)
    elif how == "blank":
        t = fx.render(recs, blanks=(0, 1, 2, 3), trail=1)
    else:
        t = fx.render(recs, fasta=True, width=60)
    with open(out, "wb") as f:
        f.write(t)
    return out


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    assert os.path.exists(CLI), "chromap-amd not built (make -C chromap_amd/csrc)"
    cache = {}

    def get(fa):
        if fa not in cache:
            idx = str(tmp_path_factory.mktemp("idx") / "d.idx")
            subprocess.run([CLI, "-i", "-r", fa, "-o", idx], check=True, stderr=subprocess.PIPE)
            cache[fa] = idx
        return cache[fa]
    return get


@pytest.mark.parametrize("name,how", [("s2_atac_q0", "wrapped"), ("s2_atac_q0", "blank"), ("s2_atac_q0", "fasta"), ("h2_hic_q0", "wrapped"),
                                      ("h2_hic_q0", "blank"), ("h2_hic_q0", "fasta"), ("s1_chip_sam", "wrapped"), ("s1_chip_sam", "blank")])
def test_cli_reproduces_the_golden_output_from_relaid_inputs(name, how, built, tmp_path):
    meta = ds.case_meta(name)
    fa, r1, r2 = ds.case_inputs(name)
    a, b = _relayout(r1, str(tmp_path / "r1.txt"), how), _relayout(r2, str(tmp_path / "r2.txt"), how)
    outs = {}
    for tag, extra in (("device", []), ("host", ["--host-ingest"])):
        out = str(tmp_path / (tag + ".out"))
        env = dict(os.environ, CM_CLI_TIMES="1")
        r = subprocess.run([CLI] + list(meta["chromap_flags"]) + extra + ["-x", built(fa), "-r", fa, "-1", a, "-2", b, "-o", out], stderr=subprocess.PIPE, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs[tag] = open(out, "rb").read()
        if tag == "device":
            assert b"[times] layout 0 free" in r.stderr and b"[times] layout 1 free" in r.stderr
    assert hashlib.md5(outs["device"]).hexdigest() == meta["bed_md5"]
    assert outs["device"] == outs["host"]


def test_cli_messages_for_fasta_with_sam_and_truncated_qualities(built, tmp_path):
    name = "s1_chip_sam"
    meta = ds.case_meta(name)
    fa, r1, r2 = ds.case_inputs(name)
    a, b = _relayout(r1, str(tmp_path / "r1.fa"), "fasta"), _relayout(r2, str(tmp_path / "r2.fa"), "fasta")
    out = str(tmp_path / "o.sam")
    r = subprocess.run([CLI] + list(meta["chromap_flags"]) + ["-x", built(fa), "-r", fa, "-1", a, "-2", b, "-o", out], stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"reference cannot write SAM for FASTA" in r.stderr
    # a four-line run reports the four-line path
    env = dict(os.environ, CM_CLI_TIMES="1")
    r = subprocess.run([CLI] + list(meta["chromap_flags"]) + ["-x", built(fa), "-r", fa, "-1", r1, "-2", r2, "-o", out], stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0 and b"[times] layout 0 strict" in r.stderr and b"] layout 0 free" not in r.stderr and b"] layout 1 free" not in r.stderr
    # a quality cut short: the reference's message for a damaged file
    recs = _records(r1)
    recs[5] = (recs[5][0], recs[5][1], recs[5][2][:-3])
    cut = str(tmp_path / "cut.fq")
    open(cut, "wb").write(fx.render(recs, width=33))
    r = subprocess.run([CLI, "--preset", "chip", "-x", built(fa), "-r", fa, "-1", cut, "-2", r2, "-o", out], stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"Didn't reach the end of sequence file, which might be corrupted!" in r.stderr
    junk = str(tmp_path / "junk.fq")
    open(junk, "wb").write(open(r1, "rb").read().replace(b"\n@", b"\nxx\n@", 1))
    r = subprocess.run([CLI, "--preset", "chip", "-x", built(fa), "-r", fa, "-1", junk, "-2", r2, "-o", out], stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"rerun with --host-ingest" in r.stderr


@pytest.mark.parametrize("how", ["wrapped", "fasta"])
def test_large_relaid_files_equal_the_reference_binary(how, tmp_path):
    """200 000 pairs, wrapped FASTQ and wrapped FASTA: BED and pairs byte-equal to the reference binary's"""
    if not os.path.exists(REF):
        pytest.skip("built reference binary not present")
    for tag, flags, gen in (("bed", ["--preset", "chip"], ["--readlen", "100", "--seed", "909", "--indel", "0.003", "--sub", "0.02"]),
                            ("pairs", ["--preset", "hic"], ["--readlen", "150", "--frag-min", "300", "--frag-max", "800", "--hic", "--seed", "910"])):
        pre = str(tmp_path / tag)
        subprocess.check_call([sys.executable, GEN, "--out", pre, "--genome", "20000000", "--chroms", "6", "--pairs", "200000"] + gen)
        idx = pre + ".idx"
        subprocess.run([CLI, "-i", "-r", pre + ".fa", "-o", idx], check=True, stderr=subprocess.PIPE)
        assert len(_records(pre + "_1.fq")) >= 200000
        a, b = _relayout(pre + "_1.fq", pre + "_1.x", how), _relayout(pre + "_2.fq", pre + "_2.x", how)
        common = flags + ["-x", idx, "-r", pre + ".fa", "-1", a, "-2", b]
        r = subprocess.run([REF] + common + ["-o", pre + ".ref", "-t", "16"], stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        g = subprocess.run([CLI] + common + ["-o", pre + ".gpu"], stderr=subprocess.PIPE)
        assert g.returncode == 0, g.stderr.decode()[-2000:]
        assert os.path.getsize(pre + ".ref") > 1000000, tag
        assert ds.md5(pre + ".gpu") == ds.md5(pre + ".ref"), tag
