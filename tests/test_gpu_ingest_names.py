"""Read names in the device FASTQ ingest (cm_ingest.hip: k_fq_name_len / k_fq_name_gather, the run-wide name store) and the pairs
text rendered from them (cmgpu_store_format_pairs_resident): the names must be kseq's (`name.s`: the header after '@' up to the first
isspace() byte) for any chunking of the text, plain or BGZF; the pairs files of `--preset hic` / `--pairs` runs, which now go through
the device ingest, must equal the host parser's and the reference's byte for byte."""
import os
import struct
import subprocess
import threading
import zlib

import numpy as np
import pytest

import datasets
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")


def _gpu():
    from chromap_amd import ChromapGPU
    fa, _, _ = datasets.case_inputs("toy_chip")
    return ChromapGPU(datasets.case_index("toy_chip"), fa, preset="chip")


def _bgzf_block(data, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def _bgzf_blocks(text, block, level=6):
    return [_bgzf_block(text[i:i + block], level) for i in range(0, len(text), block)] + [_bgzf_block(b"")]


def _bgzf_file(src, dst, block=0xff00, level=6):
    with open(dst, "wb") as f:
        f.write(b"".join(_bgzf_blocks(open(src, "rb").read(), block, level)))


def _ingest_names(g, text, chunk, limit=None, keep=True):
    """feeds `text` to stream 0 in chunks of `chunk` bytes, commits every take as a single-end batch with consecutive read ids;
    returns (records committed, bases, lengths)"""
    g.names_clear()
    g.fastq_keep_names(0, keep)
    bases, lens = [], []
    pos, carry, total = 0, b"", 0
    while True:
        piece = text[pos:pos + chunk]
        pos += len(piece)
        final = pos >= len(text)
        buf = carry + piece
        n = g.fastq_scan(0, buf, final)
        if limit:
            n = min(n, limit)
        used = g.fastq_take(0, n)
        if n:
            g.fastq_commit(n, first_read_id=total, paired=False)
            b1, o1, _, _ = g.download_batch(n)
            bases.append(b1.copy())
            lens.append(np.diff(o1))
            total += n
        carry = buf[used:]
        if final and (n == 0 or not carry.strip()):
            assert carry.strip() == b""
            break
    return total, (np.concatenate(bases) if bases else np.zeros(0, np.uint8)), (np.concatenate(lens) if lens else np.zeros(0, np.uint32))


def _ingest_names_bgzf(g, blocks, per_call, limit=None):
    g.names_clear()
    g.fastq_keep_names(0, True)
    at, total = 0, 0
    while True:
        piece = b"".join(blocks[at:at + per_call])
        at += per_call
        final = at >= len(blocks)
        n = g.fastq_scan(0, piece, final, bgzf=True)
        if limit:
            n = min(n, limit)
        g.fastq_take(0, n)
        if n:
            g.fastq_commit(n, first_read_id=total, paired=False)
            total += n
        if final and n == 0:
            break
    return total


def _check_store(g, want):
    got = g.download_names()
    assert len(got) == len(want)
    assert got == want
    assert g.names_info() == (len(want), sum(len(x) for x in want), 0)


# ---- 1. names equal kseq's for any chunking
@pytest.mark.parametrize("case", ["s2_atac_q0", datasets.HIC_CASES[0]])
def test_names_equal_kseq_for_any_chunking(case):
    g = _gpu()
    _, r1, _ = datasets.case_inputs(case)
    text = open(r1, "rb").read()
    want = ol.read_names(r1)
    assert len(want) > 1000
    for chunk, limit in ((1 << 30, None), (100003, None), (4096, None), (1 << 20, 777)):
        total, _, _ = _ingest_names(g, text, chunk, limit)
        assert total == len(want)
        _check_store(g, want)
    for block, per_call, limit in ((1 << 16, 1 << 20, None), (1 << 16, 3, 777), (4096, 50, None), (4096, 7, 777)):
        assert _ingest_names_bgzf(g, _bgzf_blocks(text, block), per_call, limit) == len(want)
        _check_store(g, want)
    g.close()


# ---- 2. header shapes
_LONG = bytes(b"abcdefghijklmnopqrstuvwxyz0123456789:/#"[i % 39] for i in range(300))
# (header line without the '@', kseq's name, sequence, quality)
_SHAPES = [
    (b"r0 a comment", b"r0", b"ACGTACGT", b"IIIIIIII"),
    (b"r1\ttab comment", b"r1", b"ACGTN", b"IIIII"),
    (b"r2", b"r2", b"AC", b"@I"),                       # a quality line that starts with '@' in front of the next header
    (b"", b"", b"ACGTACGTAC", b"@@@@@@@@@@"),           # an empty name, nothing behind it
    (b" only a comment", b"", b"GGGG", b"IIII"),        # an empty name, a comment behind it
    (b"x", b"x", b"T", b"@"),
    (_LONG, _LONG, b"ACGT" * 10, b"F" * 40),
    (b"skipped_empty_sequence extra", None, b"", b""),  # position 7: no record, no name
    (_LONG + b" " + _LONG, _LONG, b"ACGT", b"@III"),
    (b"vt\x0bvertical tab", b"vt", b"ACG", b"III"),
    (b"ff\x0cform feed", b"ff", b"ACG", b"III"),
    (b"with@at@signs/1 c", b"with@at@signs/1", b"A" * 33, b"@" * 33),
    (b"sixteen_bytes_16", b"sixteen_bytes_16", b"ACGT", b"IIII"),
    (b"fifteen_bytes_5 ", b"fifteen_bytes_5", b"ACGT", b"IIII"),
    (b"last_is_empty", None, b"", b""),                 # last: no record, no name
]
_SHAPES_WANT = [b"r0", b"r1", b"r2", b"", b"", b"x", _LONG, _LONG, b"vt", b"ff", b"with@at@signs/1", b"sixteen_bytes_16", b"fifteen_bytes_5"]


@pytest.mark.parametrize("nl", [b"\n", b"\r\n"])
@pytest.mark.parametrize("final_newline", [True, False])
def test_header_shapes(nl, final_newline):
    assert [w for _, w, _, _ in _SHAPES if w is not None] == _SHAPES_WANT
    assert _SHAPES[7][1] is None and _SHAPES[-1][1] is None
    text = b"".join(b"@" + h + nl + s + nl + b"+" + nl + q + nl for h, _, s, q in _SHAPES)
    if not final_newline:
        text = text[:-len(nl)]
    g = _gpu()
    for chunk in (1 << 20, 97):
        total, bases, lens = _ingest_names(g, text, chunk)
        assert total == len(_SHAPES_WANT)
        _check_store(g, _SHAPES_WANT)
        assert bases.tobytes() == b"".join(s for _, _, s, _ in _SHAPES)
        assert list(lens) == [len(s) for _, _, s, _ in _SHAPES if s]
    assert _ingest_names_bgzf(g, _bgzf_blocks(text, 61), 5) == len(_SHAPES_WANT)
    _check_store(g, _SHAPES_WANT)
    g.close()


# ---- 3. off means off
def test_off_means_off():
    g = _gpu()
    _, r1, _ = datasets.case_inputs("s2_atac_q0")
    text = open(r1, "rb").read()
    want_b, want_o = ol.read_fastx(r1)
    total, bases, lens = _ingest_names(g, text, 100003, keep=False)
    assert total == len(want_o) - 1
    assert g.names_info()[:2] == (0, 0) and g.download_names() == []
    assert np.array_equal(bases, want_b) and np.array_equal(lens, np.diff(want_o))
    # ... and with names on the batch arrays are the same
    total, bases, lens = _ingest_names(g, text, 100003, keep=True)
    assert np.array_equal(bases, want_b) and np.array_equal(lens, np.diff(want_o))
    assert g.names_info()[0] == total
    # turned off again: the next run keeps nothing
    _ingest_names(g, text, 1 << 30, keep=False)
    assert g.names_info()[:2] == (0, 0)
    g.close()


# ---- 4. overlap: the next batch (names included) is scanned and taken while the last one is mapped
def test_names_of_the_next_batch_taken_while_the_last_is_mapped():
    from chromap_amd import ChromapGPU, Stats
    case = "s1_atac"
    meta = datasets.case_meta(case)
    fa, r1, r2 = datasets.case_inputs(case)
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    t1, t2 = open(r1, "rb").read(), open(r2, "rb").read()
    n_all = t1.count(b"\n") // 4
    half = n_all // 2

    def cut(t, n):
        pos = 0
        for _ in range(4 * n):
            pos = t.index(b"\n", pos) + 1
        return t[:pos], t[pos:]
    a1, b1 = cut(t1, half)
    a2, b2 = cut(t2, half)

    # sequential
    g = ChromapGPU(datasets.case_index(case), fa, preset=preset, **kw)
    g.fastq_keep_names(0, True)
    g.store_clear()
    for (x1, x2, first) in ((a1, a2, 0), (b1, b2, half)):
        n = g.fastq_scan(0, x1, True)
        assert g.fastq_scan(1, x2, True) == n
        g.fastq_take(0, n); g.fastq_take(1, n)
        g.fastq_commit(n, first_read_id=first, paired=True)
        g.map_resident(Stats())
        g.store_append_resident()
    g.store_format()
    want_text, want_names = g.store_text(), g.download_names()
    g.close()
    assert want_names == ol.read_names(r1)

    g = ChromapGPU(datasets.case_index(case), fa, preset=preset, **kw)
    g.fastq_keep_names(0, True)
    g.store_clear()
    n = g.fastq_scan(0, a1, True)
    assert g.fastq_scan(1, a2, True) == n
    g.fastq_take(0, n); g.fastq_take(1, n)
    g.fastq_commit(n, first_read_id=0, paired=True)
    err = []

    def work():
        try:
            for _ in range(3):
                g.map_resident(Stats())
            g.store_append_resident()
        except Exception as e:  # noqa: BLE001
            err.append(e)
    th = threading.Thread(target=work)
    th.start()
    m = g.fastq_scan(0, b1, True)
    assert g.fastq_scan(1, b2, True) == m
    g.fastq_take(0, m); g.fastq_take(1, m)
    th.join()
    assert not err, err
    assert g.names_info()[0] == half  # (the taken names are staged: the store holds the committed batch's only)
    g.fastq_commit(m, first_read_id=half, paired=True)
    g.map_resident(Stats())
    g.store_append_resident()
    g.store_format()
    got_text, got_names = g.store_text(), g.download_names()
    g.close()
    assert got_names == want_names
    assert got_text == want_text and len(want_text) > 1000


def _hic_gpu(case):
    from chromap_amd import ChromapGPU
    meta = datasets.case_meta(case)
    fa, r1, r2 = datasets.case_inputs(case)
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    return ChromapGPU(datasets.case_index(case), fa, preset=preset, **kw), r1, r2


def _pairs_file(g, path):
    g.write_pairs_header(path)
    g.store_write_text(path, append=True)
    return open(path, "rb").read()


# ---- 5. pairs text from resident names = golden
@pytest.mark.parametrize("case", datasets.HIC_CASES)
def test_pairs_text_from_resident_names_equals_golden(case, tmp_path):
    from chromap_amd import Stats
    g, r1, r2 = _hic_gpu(case)
    g.fastq_keep_names(0, True)
    n = g.fastq_scan(0, open(r1, "rb").read(), True)
    assert g.fastq_scan(1, open(r2, "rb").read(), True) == n
    g.fastq_take(0, n); g.fastq_take(1, n)
    g.fastq_commit(n, first_read_id=0, paired=True)
    g.map_resident(Stats())
    g.store_clear()
    g.store_append_resident()
    lines, nbytes = g.store_format_pairs_resident()
    got = _pairs_file(g, str(tmp_path / "d.pairs"))
    g.close()
    want = datasets.case_golden_bed(case)
    assert got == want
    assert lines == sum(1 for ln in want.split(b"\n") if ln and not ln.startswith(b"#")) and lines > 100


# ---- 6. several batches; a gap in the read ids
def test_several_batches_and_a_gap(tmp_path):
    from chromap_amd import ChromapError, Stats
    case = datasets.HIC_CASES[0]
    g, r1, r2 = _hic_gpu(case)
    g.fastq_keep_names(0, True)
    g.store_clear()
    t1, t2 = open(r1, "rb").read(), open(r2, "rb").read()
    done = 0
    c1, c2 = t1, t2
    while True:
        n = g.fastq_scan(0, c1, True)
        assert g.fastq_scan(1, c2, True) == n
        n = min(n, 5000)
        if n == 0:
            break
        u1 = g.fastq_take(0, n)
        u2 = g.fastq_take(1, n)
        g.fastq_commit(n, first_read_id=done, paired=True)
        g.map_resident(Stats())
        g.store_append_resident()
        done += n
        c1, c2 = c1[u1:], c2[u2:]
        if not c1.strip():
            break
    names = ol.read_names(r1)
    assert done == len(names) and done > 3 * 5000
    assert g.download_names() == names
    lines, _ = g.store_format_pairs_resident()
    got = _pairs_file(g, str(tmp_path / "resident.pairs"))
    lines2, _ = g.store_format_pairs(names)
    want = _pairs_file(g, str(tmp_path / "host.pairs"))
    assert got == want and lines == lines2 and lines > 100
    # a batch that does not continue the store's read ids is refused, and nothing is committed
    n = g.fastq_scan(0, t1, True)
    g.fastq_scan(1, t2, True)
    g.fastq_take(0, 100); g.fastq_take(1, 100)
    with pytest.raises(ChromapError, match="consecutive read ids"):
        g.fastq_commit(100, first_read_id=done + 1, paired=True)
    assert g.names_info() == (done, sum(len(x) for x in names), 0)
    g.fastq_commit(100, first_read_id=done, paired=True)  # the same take, at the right read id
    assert g.download_names() == names + names[:100]
    g.close()


# ---- 7. the command line: pairs runs go through the device ingest
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


def _run_cli(args, out, extra=()):
    r = subprocess.run([CLI] + list(args) + list(extra) + ["-o", out], stderr=subprocess.PIPE, env=dict(os.environ, CM_CLI_TIMES="1"))
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    return open(out, "rb").read(), r.stderr


@pytest.mark.parametrize("case", datasets.HIC_CASES + ["s1_atac:--pairs"])
def test_cli_pairs_runs_use_the_device_ingest(case, built, tmp_path):
    golden = None
    if case.endswith(":--pairs"):  # --pairs on the ordinary (non-split) pairing of a paired golden input
        fa, r1, r2 = datasets.case_inputs(case.split(":")[0])
        flags = ["--pairs", "-q", "0"]
    else:
        fa, r1, r2 = datasets.case_inputs(case)
        flags = list(datasets.case_meta(case)["chromap_flags"])
        golden = datasets.case_golden_bed(case)
        for of in ("--chr-order", "--pairs-natural-chr-order"):  # the golden metadata keeps the order as a comma list; the program reads a file
            if of in flags:
                k = flags.index(of)
                order = str(tmp_path / (of.strip("-") + ".txt"))
                with open(order, "w") as f:
                    f.write("\n".join(flags[k + 1].split(",")) + "\n")
                flags[k + 1] = order
    idx = built(fa)
    n_reads = open(r1, "rb").read().count(b"\n") // 4
    z1, z2 = str(tmp_path / "r1.fq.gz"), str(tmp_path / "r2.fq.gz")
    _bgzf_file(r1, z1, 0xff00, 6)
    _bgzf_file(r2, z2, 30011, 1)
    host, host_err = _run_cli(flags + ["-x", idx, "-r", fa, "-1", r1, "-2", r2], str(tmp_path / "host.pairs"), ["--host-ingest"])
    assert b"[times] names" not in host_err
    assert host.count(b"\n") > 100
    for tag, a, b in (("text", r1, r2), ("bgzf", z1, z2)):
        got, err = _run_cli(flags + ["-x", idx, "-r", fa, "-1", a, "-2", b], str(tmp_path / (tag + ".pairs")))
        counts = [int(ln.split()[2]) for ln in err.decode().split("\n") if ln.startswith("[times] names ")]
        assert counts and sum(counts) == n_reads, (tag, err.decode()[-800:])
        assert got == host, tag
        if golden is not None:
            assert got == golden, tag
