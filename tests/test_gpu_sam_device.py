"""--SAM through the device ingest: whole reads kept in HBM (cm_ingest.hip: cmgpu_fastq_keep_reads, the run-wide read store), the SAM
record store and the sort / duplicate / filter / text kernels (cm_sam_post.hip).  The reads must be kseq's for any chunking of the
text, plain or BGZF; the text must equal the reference's golden files, the host writer (which the existing tests pin to the
reference) under every duplicate rule and filter, and the files of `--host-ingest` runs of the command line."""
import ctypes as C
import hashlib
import os
import struct
import subprocess
import sys
import threading
import zlib

import numpy as np
import pytest

import datasets
import oracle_lib as ol

pytestmark = pytest.mark.gpu
CLI = os.path.join(datasets.ROOT, "chromap_amd", "chromap-amd")
REF = os.path.join(datasets.ROOT, "oracle", "_ref", "chromap")


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


def _case_gpu(case):
    from chromap_amd import ChromapGPU
    meta = datasets.case_meta(case)
    fa, r1, r2 = datasets.case_inputs(case)
    preset, kw = datasets.flags_to_params(meta["chromap_flags"])
    return ChromapGPU(datasets.case_index(case), fa, preset=preset, **kw), r1, r2


def _ingest(g, texts, chunk=1 << 30, limit=None, keep=True, block=None, per_call=None, on_batch=None):
    """feeds the files' texts (read 1[, read 2]) to streams 0[, 1] -- plain text in chunks of `chunk` bytes, or BGZF blocks of `block`
    bytes, `per_call` of them per scan -- and commits every take with consecutive read ids; returns the records committed"""
    g.reads_clear()
    g.fastq_keep_reads(keep)
    m = len(texts)
    blocks = [_bgzf_blocks(t, block) for t in texts] if block else None
    at, pos, carry, buf, total = [0] * m, [0] * m, [b""] * m, [b""] * m, 0
    while True:
        cnt, fin = [], []
        for s in range(m):
            if block:
                piece = b"".join(blocks[s][at[s]:at[s] + per_call])
                at[s] += per_call
                fin.append(at[s] >= len(blocks[s]))
                cnt.append(g.fastq_scan(s, piece, fin[s], bgzf=True))
            else:
                piece = texts[s][pos[s]:pos[s] + chunk]
                pos[s] += len(piece)
                fin.append(pos[s] >= len(texts[s]))
                buf[s] = carry[s] + piece
                cnt.append(g.fastq_scan(s, buf[s], fin[s]))
        n = min(cnt)
        if limit:
            n = min(n, limit)
        for s in range(m):
            used = g.fastq_take(s, n)
            carry[s] = buf[s][used:]
        if n:
            g.fastq_commit(n, first_read_id=total, paired=m == 2)
            if on_batch:
                on_batch(n)
            total += n
        if all(fin) and (n == 0 or (not block and not any(c.strip() for c in carry))):
            break
    return total


def _want_reads(path, fmt=None):
    names = ol.read_names(path)
    b, q, off = ol.read_fastq_qual(path)
    b, q = np.asarray(b, np.uint8), np.asarray(q, np.uint8)
    if fmt:  # one [start, end] range on the - strand: reverse complement / reversed qualities of the range
        st, en = fmt
        comp = np.full(256, ord("N"), np.uint8)
        for x, y in zip(b"ACGTacgt", b"TGCATGCA"):
            comp[x] = y
        bb, qq, oo = [], [], [0]
        for i in range(len(off) - 1):
            s = b[off[i]:off[i + 1]][st:en + 1]
            t = q[off[i]:off[i + 1]][st:en + 1]
            bb.append(comp[s][::-1])
            qq.append(t[::-1])
            oo.append(oo[-1] + len(s))
        b, q, off = np.concatenate(bb), np.concatenate(qq), np.array(oo, np.uint64)
    return names, b, q, np.asarray(off, np.uint64)


def _check_reads(g, mate, want):
    names, b, q, off = g.download_reads(mate)
    assert len(names) == len(want[0]) and names == want[0]
    assert np.array_equal(off, want[3])
    assert np.array_equal(b, want[1])
    assert np.array_equal(q, want[2])
    assert g.reads_info(mate) == (len(want[0]), sum(len(x) for x in want[0]), len(want[1]), 0)


# ---- 1. reads in HBM equal kseq's for any chunking
@pytest.mark.parametrize("case", ["s2_atac_q0", datasets.HIC_CASES[0]])
def test_reads_equal_kseq_for_any_chunking(case):
    g, r1, r2 = _case_gpu(case)
    texts = [open(r1, "rb").read(), open(r2, "rb").read()]
    want = [_want_reads(r1), _want_reads(r2)]
    assert len(want[0][0]) > 1000
    for chunk, limit in ((1 << 30, None), (100003, None), (4096, None), (1 << 20, 777)):
        assert _ingest(g, texts, chunk, limit) == len(want[0][0])
        for m in range(2):
            _check_reads(g, m, want[m])
    for block, per_call, limit in ((65536, 1 << 20, None), (65536, 3, 777), (4096, 50, None)):
        assert _ingest(g, texts, limit=limit, block=block, per_call=per_call) == len(want[0][0])
        for m in range(2):
            _check_reads(g, m, want[m])
    if not datasets.is_hic(case):  # single-end (no split alignment): only read 1 is kept
        assert _ingest(g, texts[:1], 100003) == len(want[0][0])
        _check_reads(g, 0, want[0])
        assert g.reads_info(1)[0] == 0
    g.close()


def _varied_qualities(src, dst, salt=0):
    """the golden inputs carry one quality letter throughout; a copy whose quality varies along the read and from read to read, so
    that a reversal (or a missing one) shows"""
    lines = open(src, "rb").read().split(b"\n")
    for i in range(3, len(lines), 4):
        lines[i] = bytes(33 + (i + salt + 7 * k) % 41 for k in range(len(lines[i])))
    with open(dst, "wb") as f:
        f.write(b"\n".join(lines))
    return dst


def test_read_format_with_a_minus_strand_reverses_the_qualities(tmp_path):
    g, src1, r2 = _case_gpu("s2_atac_q0")
    r1 = _varied_qualities(src1, str(tmp_path / "varied_1.fq"))
    texts = [open(r1, "rb").read(), open(r2, "rb").read()]
    st = (C.c_int32 * 1)(3)
    en = (C.c_int32 * 1)(30)
    assert g.L.cmgpu_fastq_set_format(g.ctx, 0, 1, C.cast(st, C.c_void_p), C.cast(en, C.c_void_p), b"-") == 0
    want = [_want_reads(r1, (3, 30)), _want_reads(r2)]
    plain = _want_reads(r1)
    k = int(want[0][3][1])
    assert np.array_equal(want[0][2][:k], plain[2][3:31][::-1]) and not np.array_equal(want[0][2][:k], plain[2][3:31])
    assert want[0][0] == plain[0]  # names untouched
    for kw in (dict(chunk=100003), dict(block=4096, per_call=50)):
        assert _ingest(g, texts, **kw) == len(want[0][0])
        for m in range(2):
            _check_reads(g, m, want[m])
    g.close()


def test_keep_reads_off_means_off():
    g, r1, r2 = _case_gpu("s2_atac_q0")
    texts = [open(r1, "rb").read(), open(r2, "rb").read()]
    seen = {}
    for keep in (False, True):
        got = []

        def grab(n):
            b1, o1, b2, o2 = g.download_batch(n)
            got.append((b1.copy(), np.diff(o1), b2.copy(), np.diff(o2)))
        total = _ingest(g, texts, 100003, keep=keep, on_batch=grab)
        seen[keep] = [np.concatenate([x[k] for x in got]) for k in range(4)]
        if not keep:
            for m in range(2):
                assert g.reads_info(m)[:3] == (0, 0, 0)
                assert g.download_reads(m)[0] == []
        else:
            assert g.reads_info(0)[0] == total == g.reads_info(1)[0]
    for k in range(4):
        assert np.array_equal(seen[False][k], seen[True][k])
    wb, wo = ol.read_fastx(r1)
    assert np.array_equal(seen[True][0], wb) and np.array_equal(seen[True][1], np.diff(wo))
    g.close()


def test_truncated_quality_and_the_exclusion_of_names():
    from chromap_amd import ChromapError
    g, _, _ = _case_gpu("s2_atac_q0")
    text = b"@a\nACGTACGT\n+\nIIIIIIII\n@b\nACGTACGT\n+\nIIII\n@c\nACGT\n+\nIIII\n"
    g.fastq_keep_reads(False)
    assert g.fastq_scan(0, text, True) == 3  # off: the qualities of reads are not looked at
    g.fastq_keep_reads(True)
    with pytest.raises(ChromapError, match="truncated quality"):
        g.fastq_scan(0, text, True)
    with pytest.raises(ChromapError):
        g.fastq_keep_names(0, True)
    g.fastq_keep_reads(False)
    g.fastq_keep_names(0, True)
    with pytest.raises(ChromapError):
        g.fastq_keep_reads(True)
    g.close()


# ---- 2. text equals the golden file
def _sam_file(g, path):
    g.write_sam_header(path)
    g.store_write_text(path, append=True)
    return open(path, "rb").read()


def _golden(case, group, tmp_path):
    from chromap_amd import Stats
    meta = datasets.case_meta(case)
    g, r1, r2 = _case_gpu(case)
    if group:
        g.set_option("sam_format_group", group)
    mate = datasets.single_end_mate(case)
    files = [r1 if mate == 1 else r2] if mate else [r1, r2]
    bc_len = 0
    g.fastq_keep_reads(True)
    n = g.fastq_scan(0, open(files[0], "rb").read(), True)
    if not mate:
        assert g.fastq_scan(1, open(files[1], "rb").read(), True) == n
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
    k = g.sam_store_append_resident()
    assert g.sam_store_info()[0] == k and k > 100
    lines, nbytes = g.store_format_sam(barcode_length=bc_len)
    got = _sam_file(g, str(tmp_path / "d.sam"))
    g.close()
    want = datasets.case_golden_bed(case)
    assert hashlib.md5(got).hexdigest() == meta["bed_md5"]
    assert got == want
    assert lines == meta["reference_stderr_counters"]["num_output"]
    assert nbytes == sum(len(ln) + 1 for ln in want.split(b"\n") if ln and not ln.startswith(b"@SQ"))


@pytest.mark.parametrize("case", datasets.SAM_CASES + datasets.HIC_SAM_CASES + datasets.SAM_BC_CASES)
def test_sam_text_from_the_device_equals_golden(case, tmp_path):
    _golden(case, None, tmp_path)


@pytest.mark.parametrize("group", [16, 64])
@pytest.mark.parametrize("case", [datasets.SAM_CASES[0], datasets.HIC_SAM_CASES[0], datasets.SAM_BC_CASES[0]])
def test_sam_text_with_the_other_group_widths(case, group, tmp_path):
    """the format kernel's group width is a measurement knob (8, 16 or 64 lanes per line): same bytes"""
    _golden(case, group, tmp_path)


# ---- 3. several batches, duplicate rules, filter: the host writer on the same records
def test_several_batches_duplicate_rules_and_filter(tmp_path):
    from chromap_amd import Stats, _capi
    from chromap_amd._capi import SamRecord
    case = "s3_sam_q0"
    g, src1, src2 = _case_gpu(case)
    # (qualities that vary along the read: the QUAL column of a read on the - strand is then the reverse of the file's, and differs from it)
    r1 = _varied_qualities(src1, str(tmp_path / "varied_1.fq"))
    r2 = _varied_qualities(src2, str(tmp_path / "varied_2.fq"), salt=17)
    texts = [open(r1, "rb").read(), open(r2, "rb").read()]
    parts = []
    g.sam_store_clear()

    def on_batch(n):
        g.map_resident(Stats())
        parts.append(g.download_sam())
        g.sam_store_append_resident()
    total = _ingest(g, texts, limit=5000, on_batch=on_batch)
    assert total > 3 * 5000 and len(parts) > 3
    md_cap = parts[0][3]
    assert all(p[3] == md_cap for p in parts)
    slots = sum(p[4] for p in parts)
    assert slots == 2 * total
    rec = (SamRecord * slots)()
    at = 0
    for p in parts:
        C.memmove(C.byref(rec, at * C.sizeof(SamRecord)), p[0], p[4] * C.sizeof(SamRecord))
        at += p[4]
    cigar = np.concatenate([p[1][:p[4] * _capi.SAM_CIGAR_CAP] for p in parts])
    md = np.concatenate([p[2][:p[4] * md_cap] for p in parts])
    sam = (rec, cigar, md, md_cap, slots)
    # the two duplicate rules must be told apart: runs of operator== with two or more distinct MAPQ values
    runs = {}
    for i in range(slots):
        r = rec[i]
        if r.valid:
            runs.setdefault((r.rid, r.pos, r.flag & 64, r.mrid, r.mpos), set()).add(r.mapq)
    mixed = sum(1 for v in runs.values() if len(v) >= 2)
    print("runs of equal (rid, pos, flag & 64, mrid, mpos) with two or more MAPQ values:", mixed)
    assert mixed >= 10
    assert g.sam_store_info()[0] == sum(1 for i in range(slots) if rec[i].valid)
    n1, n2 = ol.read_names(r1), ol.read_names(r2)
    b1, q1, o1 = ol.read_fastq_qual(r1)
    b2, q2, o2 = ol.read_fastq_qual(r2)
    header = b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (nm, ln) for nm, ln in zip(g.names, g.reference_lengths()))
    texts_seen = {}
    for dedup in (0, 1):
        for lowmem in (0, 1):
            for thr in (0, 30):
                p = _capi.Params.from_buffer_copy(g.params)
                p.remove_pcr_duplicates, p.low_memory_mode, p.mapq_threshold = dedup, lowmem, thr
                out = str(tmp_path / "h.sam")
                want_lines = g.write_sam(sam, True, n1, n2, b1, q1, o1, b2, q2, o2, out, params=p)
                want = open(out, "rb").read()
                assert want.startswith(header)
                lines, nbytes = g.store_format_sam(params=p)
                got = g.store_text()
                assert lines == want_lines and nbytes == len(got), (dedup, lowmem, thr)
                assert got == want[len(header):], (dedup, lowmem, thr)
                texts_seen[(dedup, lowmem, thr)] = got
    assert texts_seen[(1, 0, 0)] != texts_seen[(1, 1, 0)]  # (the rules select different survivors here)
    # the golden file was made from one-letter qualities: every column but QUAL must be the reference's, and QUAL must be the file's
    # qualities, reversed where the flag says the read lies on the - strand
    def cols(text):
        return [ln.split(b"\t") for ln in text.split(b"\n") if ln and not ln.startswith(b"@SQ")]
    got_cols, gold_cols = cols(texts_seen[(0, 1, 0)]), cols(datasets.case_golden_bed(case))
    assert [c[:10] + c[11:] for c in got_cols] == [c[:10] + c[11:] for c in gold_cols]
    quals = ({n: bytes(q1[o1[i]:o1[i + 1]]) for i, n in enumerate(n1)}, {n: bytes(q2[o2[i]:o2[i + 1]]) for i, n in enumerate(n2)})
    n_minus = 0
    for c in got_cols:
        flag = int(c[1])
        q = quals[1 if flag & 128 else 0][c[0]]
        assert len(c[10]) == len(c[9]) <= len(q)
        if flag & 16:
            n_minus += 1
            assert c[10] in q[::-1], c[0]  # (the first length_after_trim qualities reversed, cut to the CIGAR's query length)
            assert c[10] != q[:len(c[10])]
        else:
            assert c[10] == q[:len(c[10])], c[0]
    assert n_minus > 1000
    g.close()


def test_stores_of_different_runs_are_refused():
    """records whose reads are not in the read store: no SAM text with lines missing, CMGPU_EINVAL"""
    from chromap_amd import ChromapError, Stats
    g, r1, r2 = _case_gpu("s1_chip_sam")
    t1, t2 = open(r1, "rb").read(), open(r2, "rb").read()
    g.sam_store_clear()
    _ingest(g, [t1, t2], limit=5000, on_batch=lambda n: (g.map_resident(Stats()), g.sam_store_append_resident()))
    lines, _ = g.store_format_sam()
    assert lines > 1000
    # a new run's reads (the first 5 000 only) under the old run's records
    g.reads_clear()
    g.fastq_scan(0, t1, True); g.fastq_scan(1, t2, True)
    g.fastq_take(0, 5000); g.fastq_take(1, 5000)
    g.fastq_commit(5000, first_read_id=0, paired=True)
    with pytest.raises(ChromapError, match="not of one run"):
        g.store_format_sam()
    assert g.store_text() == b""
    g.close()


# ---- 4. overlap: the next batch is scanned and taken while the last one is mapped and stored
def test_next_batch_taken_while_the_last_is_mapped_and_stored():
    from chromap_amd import Stats
    case = "s1_chip_sam"
    _, r1, r2 = datasets.case_inputs(case)
    t1, t2 = open(r1, "rb").read(), open(r2, "rb").read()
    half = (t1.count(b"\n") // 4) // 2

    def cut(t, n):
        pos = 0
        for _ in range(4 * n):
            pos = t.index(b"\n", pos) + 1
        return t[:pos], t[pos:]
    a1, b1 = cut(t1, half)
    a2, b2 = cut(t2, half)

    g, _, _ = _case_gpu(case)
    g.fastq_keep_reads(True)
    for (x1, x2, first) in ((a1, a2, 0), (b1, b2, half)):
        n = g.fastq_scan(0, x1, True)
        assert g.fastq_scan(1, x2, True) == n
        g.fastq_take(0, n); g.fastq_take(1, n)
        g.fastq_commit(n, first_read_id=first, paired=True)
        g.map_resident(Stats())
        g.sam_store_append_resident()
    g.store_format_sam()
    want = g.store_text()
    g.close()

    g, _, _ = _case_gpu(case)
    g.fastq_keep_reads(True)
    n = g.fastq_scan(0, a1, True)
    assert g.fastq_scan(1, a2, True) == n
    g.fastq_take(0, n); g.fastq_take(1, n)
    g.fastq_commit(n, first_read_id=0, paired=True)
    err = []

    def work():
        try:
            for _ in range(3):
                g.map_resident(Stats())
            g.sam_store_append_resident()
        except Exception as e:  # noqa: BLE001
            err.append(e)
    th = threading.Thread(target=work)
    th.start()
    m = g.fastq_scan(0, b1, True)
    assert g.fastq_scan(1, b2, True) == m
    g.fastq_take(0, m); g.fastq_take(1, m)
    th.join()
    assert not err, err
    assert g.reads_info(0)[0] == half  # (the taken reads are staged: the store holds the committed batch's only)
    g.fastq_commit(m, first_read_id=half, paired=True)
    g.map_resident(Stats())
    g.sam_store_append_resident()
    g.store_format_sam()
    got = g.store_text()
    g.close()
    assert got == want and len(want) > 100000
    header_len = sum(len(ln) + 1 for ln in datasets.case_golden_bed(case).split(b"\n") if ln.startswith(b"@SQ"))
    assert got == datasets.case_golden_bed(case)[header_len:]


# ---- 5. a gap in the read ids is refused, nothing is committed
def test_a_gap_in_the_read_ids_commits_nothing():
    from chromap_amd import ChromapError
    g, r1, r2 = _case_gpu("s2_atac_q0")
    t1, t2 = open(r1, "rb").read(), open(r2, "rb").read()
    want = [_want_reads(r1), _want_reads(r2)]
    g.reads_clear()
    g.fastq_keep_reads(True)
    for first, fails in ((0, False), (101, True), (100, False)):
        g.fastq_scan(0, t1, True)
        g.fastq_scan(1, t2, True)
        g.fastq_take(0, 100); g.fastq_take(1, 100)
        before = [g.reads_info(m) for m in range(2)]
        if fails:
            with pytest.raises(ChromapError, match="consecutive read ids"):
                g.fastq_commit(100, first_read_id=first, paired=True)
            assert [g.reads_info(m) for m in range(2)] == before
        else:
            g.fastq_commit(100, first_read_id=first, paired=True)
    for m in range(2):
        names, b, q, off = g.download_reads(m)
        end = int(want[m][3][100])
        assert names == want[m][0][:100] * 2
        assert np.array_equal(b, np.concatenate([want[m][1][:end]] * 2)) and np.array_equal(q, np.concatenate([want[m][2][:end]] * 2))
        assert np.array_equal(off, np.concatenate([want[m][3][:101], want[m][3][1:101] + np.uint64(end)]))
    g.close()


# ---- 6. the command line: --SAM runs go through the device ingest
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


def _read_counts(err, mate):
    return [int(ln.split()[3]) for ln in err.decode().split("\n") if ln.startswith("[times] reads %d " % mate)]


@pytest.mark.parametrize("case", ["s1_chip_sam", "s3_sam_q0", "s2_atac_sam", "s1_se_sam", "h1_hic_sam", "h2_hic_sam_q0"])
def test_cli_sam_runs_use_the_device_ingest(case, built, tmp_path):
    fa, r1, r2 = datasets.case_inputs(case)
    flags = list(datasets.case_meta(case)["chromap_flags"])
    golden = datasets.case_golden_bed(case)
    mate = datasets.single_end_mate(case)
    files = [r1 if mate == 1 else r2] if mate else [r1, r2]
    idx = built(fa)
    n_reads = open(files[0], "rb").read().count(b"\n") // 4
    zs = [str(tmp_path / ("r%d.fq.gz" % k)) for k in range(len(files))]
    for k, (src, dst) in enumerate(zip(files, zs)):
        _bgzf_file(src, dst, (0xff00, 30011)[k], (6, 1)[k])

    def reads(fs):
        return ["-1", fs[0]] + (["-2", fs[1]] if len(fs) == 2 else [])
    host, host_err = _run_cli(flags + ["-x", idx, "-r", fa] + reads(files), str(tmp_path / "host.sam"), ["--host-ingest"])
    assert b"[times] reads" not in host_err
    assert host == golden
    for tag, fs in (("text", files), ("bgzf", zs)):
        got, err = _run_cli(flags + ["-x", idx, "-r", fa] + reads(fs), str(tmp_path / (tag + ".sam")))
        for m in range(len(files)):
            counts = _read_counts(err, m + 1)
            assert counts and sum(counts) == n_reads, (tag, m, err.decode()[-800:])
        assert not _read_counts(err, len(files) + 1)
        assert got == host, tag
        assert got == golden, tag


def test_cli_sam_with_barcodes_and_the_translate_table(built, tmp_path):
    """barcoded --SAM goes through the device ingest as well; with --barcode-translate it stays on the host route"""
    case = datasets.SAM_BC_CASES[0]
    fa, r1, r2 = datasets.case_inputs(case)
    bcf, wlf = datasets.case_barcode_inputs(case)
    flags = list(datasets.case_meta(case)["chromap_flags"])
    idx = built(fa)
    args = flags + ["-x", idx, "-r", fa, "-1", r1, "-2", r2, "-b", bcf, "--barcode-whitelist", wlf]
    n_reads = open(r1, "rb").read().count(b"\n") // 4
    got, err = _run_cli(args, str(tmp_path / "dev.sam"))
    assert sum(_read_counts(err, 1)) == n_reads == sum(_read_counts(err, 2))
    assert got == datasets.case_golden_bed(case)
    table = str(tmp_path / "tr.tsv")
    with open(wlf) as f, open(table, "w") as t:
        for i, ln in enumerate(f):
            t.write("CELL%05d\t%s\n" % (i, ln.strip()))
    tr, tr_err = _run_cli(args + ["--barcode-translate", table], str(tmp_path / "tr.sam"))
    assert b"[times] reads" not in tr_err
    tr_host, _ = _run_cli(args + ["--barcode-translate", table], str(tmp_path / "tr_host.sam"), ["--host-ingest"])
    assert tr == tr_host and b"CB:Z:CELL" in tr and tr.count(b"\n") == got.count(b"\n")


# ---- 7. against the reference binary at scale
def test_instrument_shaped_million_pairs_sam(tmp_path):
    """One million pairs shaped like an instrument's output (tools/gen_real.py: read lengths mixed per read, N bases, adapter
    read-through; a reference with soft-masked segments, IUPAC codes and N runs), --preset chip --SAM: the file of the device
    route must be the reference binary's, byte for byte."""
    if not os.path.exists(REF):
        pytest.skip("built reference binary not present")
    pre = str(tmp_path / "d")
    subprocess.check_call([sys.executable, os.path.join(datasets.ROOT, "tools", "gen_real.py"), "--out", pre, "--genome", "60000000", "--chroms", "8",
                           "--pairs", "1000000", "--seed", "707"])
    idx = pre + ".idx"
    subprocess.run([CLI, "-i", "-r", pre + ".fa", "-o", idx], check=True, stderr=subprocess.PIPE)
    reads = ["-x", idx, "-r", pre + ".fa", "-1", pre + "_1.fq", "-2", pre + "_2.fq"]
    r = subprocess.run([REF, "--preset", "chip", "--SAM"] + reads + ["-o", pre + ".ref.sam", "-t", "16"], stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got, err = _run_cli(["--preset", "chip", "--SAM"] + reads, pre + ".gpu.sam")
    assert sum(_read_counts(err, 1)) == 1000000 == sum(_read_counts(err, 2))
    assert os.path.getsize(pre + ".ref.sam") > 200_000_000
    assert datasets.md5(pre + ".gpu.sam") == datasets.md5(pre + ".ref.sam")
